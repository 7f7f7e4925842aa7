"""CPU: the reference of the mesh-shadow pass (irt_shadow_mesh_cases) is sharp and sound before any GPU runs -- its caps, a float32 restatement of the rule
inside its bounds on every case, the eight mutants it must reject, the prefilter's argument on the restatement, the bit-identity geometry -- and the layers
above the kernel that need no device: pose inversion, the C-ABI's refusals, the conf key and its json form, the tool's choice of file."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import irt_shadow_mesh_cases as MC
import occlusion_cases as OC
import trace_cases as TC

F32, F64 = np.float32, np.float64
INVALID = -1                # TEXIR_ERR_INVALID
D = 8                       # a dummy non-null pointer


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MC.GPU_CASES)
def test_caps_of_every_case(name):
    r = MC.case(name).ref()
    over, unc = r.caps()
    print(name, r.summary())
    assert over == 0, "%d rays overflow a candidate list" % over
    assert unc <= MC.CAP_MULTI, "%.4f of the samples that may meet a box are uncertain" % unc
    assert r.box_pin_fails == 0, "a ray certainly hits a triangle and not certainly the box around it"


def test_the_cases_cover_what_the_issue_lists():
    cs = [MC.case(n) for n in MC.GPU_CASES]
    assert {1, 2, 63, 64, 65, 100, 128, 512} <= {c.N for c in cs} and {1, 63, 64, 65, 130} <= {len(c.ids) for c in cs}
    assert {0, 1, 2, 8} <= {c.K for c in cs} and {1, 2, 3, 8} <= {c.M for c in cs} and {1, 2} <= {len(c.occ) for c in cs} and {1, 8, 16, 32} <= {c.parts for c in cs}
    assert any(len(c.occ) == 1 and c.K == 2 for c in cs), "two instances of one handle"
    assert [MC.occluder(n).T for n in ("tri", "cube", "ico", "table", "person")] == [1, 12, 80, 60, 1984]
    assert {"tri", "cube", "ico", "table", "person"} <= {n for c in cs for n in c.occ} and {"uniform", "cosine"} <= {c.mode for c in cs}
    below, behind = MC.case("box_below").ref(), MC.case("box_behind_wall").ref()
    assert below.meet_maybe.sum() == 0, "no ray may meet a box beyond the corner under the floor"
    assert behind.meet_yes.sum() > 0 and behind.blk_maybe.sum() == 0 and not any(np.abs(m).any() for m in behind.mid), "met, never in front of the wall"
    top = MC.case("box_open_top").ref()
    assert top.meet_yes.sum() > top.q_maybe.sum() > 0 and not np.abs(top.mid[0]).any(), "the object above the open top is met by rays that leave the scene"
    enc = MC.case("box_enclosed").ref()
    assert enc.all_blocked(0).sum() >= 16 and np.array_equal(enc.all_blocked(0), enc.all_blocked(2)) and not enc.all_blocked(1).any()


@pytest.mark.parametrize("name", MC.CPU_CASES)
def test_float32_restatement_lies_inside_the_reference(name):
    c = MC.case(name)
    lost, stats = MC.shadow_mesh_f32(c)
    worst = MC.check(c, lost, stats, MC.SENTINEL, "float32 restatement")
    assert worst <= 1.0
    # the prefilter changes no bit of the restatement (and shadow_mesh_f32 asserts that it rejects no ray the leaf test accepts)
    off, _ = MC.shadow_mesh_f32(c, prefilter=False)
    assert np.array_equal(lost.view(np.uint32), off.view(np.uint32))


@pytest.mark.parametrize("mut", MC.MUTANTS)
def test_the_check_rejects_the_mutant(mut):
    c = MC.case(MC.MUTANT_CASES[mut])
    MC.check(c, *MC.shadow_mesh_f32(c), MC.SENTINEL, "unmutated")
    lost, stats = MC.shadow_mesh_f32(c, mut)
    assert TC.rejected(MC.check, c, lost, stats, MC.SENTINEL, mut), "the mutant %s passes on %s" % (mut, c.name)


def test_the_mutant_list_is_the_documented_one():
    assert len(MC.MUTANTS) == 8 and set(MC.MUTANT_CASES) == set(MC.MUTANTS)


def test_where_every_sample_is_blocked_the_restatement_is_the_estimator_bit_for_bit():
    import irt_shadow_cases as SH
    c = MC.case("box_enclosed")
    r = c.ref()
    sel = r.all_blocked(0)
    L, d, t, pid, rad = SH.traced(c)
    full = TC.estimator_f32(c.nrm[L], d, rad.reshape(len(L), c.N, 3), False, "group", c.parts)
    lost, st = MC.shadow_mesh_f32(c)
    assert np.array_equal(lost[0][L][sel].view(np.uint32), full[sel].view(np.uint32)) and (full[sel] > 0).any()
    assert np.array_equal(lost[0].view(np.uint32), lost[2].view(np.uint32)) and not lost[1][L].view(np.uint32).any()


def test_the_prefilter_passes_what_the_leaf_test_accepts_on_hard_rays():
    """rays aimed at corners and edges of a box mesh and along its faces, from far away and from a corner itself, in a pose with large coordinates: the
    float32 box test of the header never rejects a ray the float32 leaf test accepts"""
    g = MC.occluder("cube")
    rng = np.random.default_rng(11)
    corners = g.verts[rng.integers(0, 8, 4000)].astype(F64)
    mids = 0.5 * (corners + g.verts[rng.integers(0, 8, 4000)].astype(F64))
    tgt = np.concatenate([corners, mids])
    for scale, shift in ((1.0, 0.0), (1e3, 0.0), (1.0, 1e4), (1e-3, 0.0)):
        org = (tgt + rng.normal(size=tgt.shape) * scale + shift * np.array([1.0, -1.0, 0.5])).astype(F32)
        org[::7] = tgt[::7].astype(F32)                                        # from a corner itself
        d = ((tgt - org.astype(F64)) * rng.uniform(0.25, 4.0, (len(tgt), 1))).astype(F32)
        d[::5, 0] = 0                                                           # axis-parallel components
        d[1::7] = rng.normal(size=d[1::7].shape).astype(F32)
        inside, t = OC.leaf_f32(g, org, d)
        with np.errstate(invalid="ignore"):
            hit = (inside & (t > 0)).any(1)
        met = MC.box_f32(g.verts.min(0), g.verts.max(0), org, d)
        assert hit.sum() > 500 and not (hit & ~met).any()
        assert (~met).sum() > 0 or scale < 1


# ---- poses -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_pose_inversion_and_its_refusals():
    import torch
    from texir_code_amd import scene as S
    P = np.stack([MC.pose((1.0, -2.0, 3.0), (1, 2, 3), 40.0, 1.5), MC.pose(), MC.pose((0, 0, 0), (0, 0, 1), 90.0, (2.0, 0.5, 4.0))])
    W = S.world_to_object(P)
    assert W.shape == (3, 12) and W.dtype == F32
    for j in range(3):
        M4, W4 = np.eye(4), np.eye(4)
        M4[:3], W4[:3] = P[j], W[j].astype(F64).reshape(3, 4)
        assert np.abs(W4 @ M4 - np.eye(4)).max() < 1e-6
        want = np.linalg.inv(M4)[:3].astype(F32)                                 # inverted in float64, rounded once
        assert np.abs(W[j].reshape(3, 4) - want).max() <= 2.0 ** -22 * np.abs(want).max()
    assert np.array_equal(W[1], np.eye(3, 4, dtype=F32).reshape(-1))
    four = np.tile(np.eye(4), (2, 1, 1))
    four[:, :3] = P[:2]
    assert np.array_equal(S.world_to_object(four), W[:2]) and np.array_equal(S.world_to_object(torch.from_numpy(P)), W)
    sing = P.copy()
    sing[1, :, 2] = 0
    with pytest.raises(ValueError, match="pose 1 is singular"):
        S.world_to_object(sing)
    nearly = P.copy()
    nearly[2, :, :3] = np.outer([1, 2, 3], [1, 1, 1]) + 1e-14 * np.eye(3)
    with pytest.raises(ValueError, match="pose 2 is singular"):
        S.world_to_object(nearly)
    bad = P.copy()
    bad[0, 1, 3] = np.nan
    with pytest.raises(ValueError, match="pose 0 has a non-finite entry"):
        S.world_to_object(bad)
    four[1, 3, 0] = 0.5
    with pytest.raises(ValueError, match="pose 1 is not affine"):
        S.world_to_object(four)
    with pytest.raises(ValueError, match="poses must be"):
        S.world_to_object(np.zeros((2, 12)))


def test_the_rule_keeps_the_ray_parameter():
    """the float32 object-space ray of a point x + t d is o' + t d' up to rounding: an affine map keeps t"""
    c = MC.case("box_cube")
    rng = np.random.default_rng(2)
    x, d = rng.uniform(0, 8, (100, 3)).astype(F32), rng.normal(size=(100, 3)).astype(F32)
    o2, d2 = MC.point_f32(c.w2o[0], x).astype(F64), MC.dir_f32(c.w2o[0], d).astype(F64)
    far = MC.point_f32(c.w2o[0], (x.astype(F64) + 2.5 * d.astype(F64)).astype(F32)).astype(F64)
    assert np.abs(o2 + 2.5 * d2 - far).max() < 1e-4


# ---- the C-ABI's refusals, without a device --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from texir_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


_HANDLES = (C.c_void_p * 8)(*([D] * 8))
_INST = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32)
ORDER = ("scene", "pos", "nrm", "shift", "ids", "n_ids", "Nt", "N", "mode", "occ", "Q", "inst", "w2o", "K", "sets", "M", "out", "stats", "flags", "ws", "ws_bytes", "stream")


def mesh_args(**kw):
    a = dict(scene=D, pos=D, nrm=D, shift=D, ids=D, n_ids=64, Nt=100, N=64, mode=0, occ=C.cast(_HANDLES, C.c_void_p), Q=2, inst=_INST.ctypes.data_as(C.c_void_p), w2o=D, K=2,
             sets=D, M=3, out=D, stats=None, flags=0, ws=D, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ORDER)


def refused(L, msg, **kw):
    rc = L.texir_irt_shadow_mesh(*mesh_args(**kw))
    got = L.texir_last_error().decode()
    assert rc == INVALID and got.startswith("texir_irt_shadow_mesh: " + msg), (kw, rc, got)


def test_cabi_refusals(L):
    none = dict(occ=None, inst=None, w2o=None, sets=None, out=None)              # the ranges are reported before any null buffer
    refused(L, "Q must be in 0..8, got 9", Q=9, **none)
    refused(L, "Q must be in 0..8, got -1", Q=-1)
    refused(L, "K must be in 0..8, got 9", K=9, **none)
    refused(L, "K must be in 0..8, got -2", K=-2)
    refused(L, "M must be in 1..8, got 0", M=0, **dict(none, inst=_INST.ctypes.data_as(C.c_void_p)))
    refused(L, "M must be in 1..8, got 9", M=9)
    refused(L, "inst_obj is null", inst=None)
    refused(L, "inst_obj[1] = 1 names no occluder (Q = 1)", Q=1, occ=None, w2o=None, sets=None, out=None)
    bad = np.array([0, -1], np.int32)
    refused(L, "inst_obj[1] = -1 names no occluder (Q = 2)", inst=bad.ctypes.data_as(C.c_void_p))
    refused(L, "inst_obj[0] = 0 names no occluder (Q = 0)", Q=0, K=1)
    refused(L, "bad sizes N=0", N=0, occ=None, w2o=None, sets=None, out=None)
    refused(L, "bad sizes N=-3", N=-3)
    refused(L, "bad sizes", n_ids=-1)
    refused(L, "mode must be uniform(0) or cosine(1), got 2", mode=2)
    refused(L, "Nt too large", Nt=1 << 31)
    refused(L, "occluders is null", occ=None)
    holes = (C.c_void_p * 2)(D, None)
    refused(L, "occluders[1] is null", occ=C.cast(holes, C.c_void_p))
    refused(L, "inst_world_to_obj is null", w2o=None)
    refused(L, "sets is null", sets=None)
    for k in ("scene", "pos", "nrm", "shift", "out"):
        refused(L, "null argument", **{k: None})
    need = 12 * 3 * 8 * 64                                                         # 12 B x M x parts (N = 64: 8) per listed texel
    assert L.texir_irt_shadow_mesh_workspace_bytes(64, 64, 3) == need
    refused(L, "the workspace holds %d bytes, the call needs %d" % (need - 1, need), ws_bytes=need - 1)
    refused(L, "the workspace holds 0 bytes, the call needs %d" % need, ws=None)
    assert L.texir_irt_shadow_mesh(*mesh_args(n_ids=0, ws=None, ws_bytes=0)) == 0   # a non-null empty list is a no-op
    assert L.texir_irt_shadow_mesh(*mesh_args(K=0, Q=0, occ=None, inst=None, w2o=None, n_ids=0)) == 0      # K = 0 needs no matrices, Q = 0 no handles


def test_workspace_bytes(L):
    f = L.texir_irt_shadow_mesh_workspace_bytes
    assert f(1, 1, 1) == 12 and f(1, 3, 8) == 96 and f(130, 256, 5) == 12 * 5 * 32 * 130 and f(65, 128, 1) == 12 * 16 * 65
    for bad in ((0, 64, 1), (-1, 64, 1), (64, 0, 1), (64, 64, 0), (64, 64, 9)):
        assert f(*bad) == 0


# ---- the conf key, its json form, the tool ---------------------------------------------------------------------------------------------------------------------------

class _Conf(dict):
    def get(self, k, d=None):
        return dict.get(self, k, d)


def test_conf_key_and_json_forms_parse_and_bad_values_raise(tmp_path):
    from texir_code_amd import irtobject as IO_
    from texir_code_amd.conf import ConfigFactory
    assert IO_.parse("none") is None and IO_.parse(None) is None and IO_.parse(" None ") is None
    p = tmp_path / "a.conf"
    p.write_text('train {\n    irt_objects = [ { "obj": "/m/chair.obj", "pose": [[1, 0, 0, 2], [0, 1, 0, 0.5], [0, 0, 1, -3], [0, 0, 0, 1]] },\n'
                 '                    { "obj": "/m/chair.obj", "pose": { "translate": [1, 2, 3], "rotate_deg": [0, 90, 0], "scale": 2 } }, { "obj": "/m/t.obj" } ]\n'
                 "    irt_object_samples = 32\n}\n")
    conf = ConfigFactory.parse_file(str(p))
    objs = IO_.parse(conf.get(IO_.KEY, "none"))
    assert [o[0] for o in objs] == ["/m/chair.obj", "/m/chair.obj", "/m/t.obj"] and IO_.samples_setting(conf, 128) == 32 and IO_.samples_setting(_Conf(), 128) == 128
    assert np.array_equal(objs[0][1], [[1, 0, 0, 2], [0, 1, 0, 0.5], [0, 0, 1, -3]]) and np.array_equal(objs[2][1], np.eye(3, 4))
    want = np.array([[0, 0, 2, 1], [0, 2, 0, 2], [-2, 0, 0, 3]], F64)             # Ry(90) S(2), then the translation
    assert np.abs(objs[1][1] - want).max() < 1e-12
    # M = T Rz Ry Rx S on a point
    M = IO_.pose_matrix({"translate": [1, 0, 0], "rotate_deg": [90, 0, 90], "scale": [1, 2, 3]})
    assert np.abs(M @ np.array([1.0, 1.0, 1.0, 1.0]) - np.array([1 + 3, 1, 2])).max() < 1e-12
    # the same list in a json file, bare or under "objects"; relative paths are taken from the file's directory
    spec = [{"obj": "chair.obj", "pose": {"translate": [1, 2, 3]}}, {"obj": "/abs/t.obj"}]
    for k, body in enumerate((spec, {"objects": spec})):
        js = tmp_path / ("o%d.json" % k)
        js.write_text(json.dumps(body))
        got = IO_.parse(str(js))
        assert [o[0] for o in got] == [str(tmp_path / "chair.obj"), "/abs/t.obj"] and np.array_equal(got[0][1][:, 3], [1, 2, 3])
    with pytest.raises(FileNotFoundError, match="train.irt_objects = .*nothing.json: no such file"):
        IO_.parse(str(tmp_path / "nothing.json"))
    (tmp_path / "broken.json").write_text("[{")
    with pytest.raises(ValueError, match="train.irt_objects = .*broken.json: not json"):
        IO_.parse(str(tmp_path / "broken.json"))
    for bad in ([], 5, [{"pose": [[1]]}], [{"obj": "a.obj", "colour": 1}], ["a.obj"], [{"obj": "a.obj"}] * 9):
        with pytest.raises(ValueError, match="train.irt_objects"):
            IO_.parse(bad)
    for bad in ([[1, 0, 0], [0, 1, 0]], {"translate": [1, 2]}, {"rotate": [0, 0, 0]}, {"scale": [1, 2]}, [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]],
                {"translate": [0, float("nan"), 0]}, {"scale": "big"}):
        with pytest.raises(ValueError, match="train.irt_objects"):
            IO_.pose_matrix(bad)
    for bad in (0, -4, 2.5, "many", True):
        with pytest.raises(ValueError, match="train.irt_object_samples"):
            IO_.samples_setting(_Conf({"train.irt_object_samples": bad}), 64)
    assert IO_.shadow_sets(1) == [[[0]]] and IO_.shadow_sets(3) == [[[0], [1], [2], [0, 1, 2]]]
    assert IO_.shadow_sets(8) == [[[k] for k in range(8)], [list(range(8))]]


def test_object_irt_chooses_its_file_and_refuses_the_rest(tmp_path, capsys):
    from texir_code_amd import io_formats as IO, tools
    rng = np.random.default_rng(8)
    d = str(tmp_path)
    IO.write_hdr(os.path.join(d, "0_irr_texture.hdr"), rng.random((8, 8, 3), dtype=F32) + F32(0.5))
    rd = lambda n: np.asarray(IO.read_hdr(os.path.join(d, n)), F32)
    E = rd("0_irr_texture.hdr")
    dst = os.path.join(d, "0_irr_texture_objects.hdr")
    ref = str(tmp_path / "ref.hdr")

    def run(argv):
        if os.path.exists(dst):
            os.remove(dst)
        capsys.readouterr()
        rc = tools.main(["object-irt", d] + argv)
        return rc, (open(dst, "rb").read() if rc == 0 else None), capsys.readouterr().out
    rc, _, msg = run([])                                                           # no shadow files yet: the file pattern and the conf key are named
    assert rc == 1 and "0_irr_texture_object<k>_shadow.hdr" in msg and "train.irt_objects" in msg
    rc, _, msg = run(["--object", "1"])
    assert rc == 1 and "0_irr_texture_object1_shadow.hdr" in msg and "train.irt_objects" in msg
    lost = (rng.random((4, 8, 8, 3), dtype=F32) * F32(2)).astype(F32)              # beyond E on part of the image
    for k in range(3):
        IO.write_hdr(os.path.join(d, "0_irr_texture_object%d_shadow.hdr" % k), lost[k])
    rc, _, msg = run([])                                                           # three objects and no union file
    assert rc == 1 and "0_irr_texture_objects_shadow.hdr" in msg and "train.irt_objects" in msg
    IO.write_hdr(os.path.join(d, "0_irr_texture_objects_shadow.hdr"), lost[3])

    def want(name):
        IO.write_hdr(ref, np.maximum(E - rd(name), F32(0)))
        return open(ref, "rb").read()
    rc, got, _ = run([])
    assert rc == 0 and got == want("0_irr_texture_objects_shadow.hdr")
    rc, got2, _ = run(["--object", "0", "--object", "1", "--object=2"])
    assert rc == 0 and got2 == got
    rc, got, _ = run(["--object", "1"])
    assert rc == 0 and got == want("0_irr_texture_object1_shadow.hdr") and (rd("0_irr_texture_objects.hdr") >= 0).all()
    rc, _, msg = run(["--object", "0", "--object", "2"])                           # neither one nor all
    assert rc == 1 and "no other subset" in msg and "train.irt_objects" in msg
    rc, _, msg = run(["--object", "5"])
    assert rc == 1 and "0_irr_texture_object5_shadow.hdr" in msg
    assert run(["--object", "x"])[0] == 2 and run(["--object", "-1"])[0] == 2 and run(["--shadow"])[0] == 2
    run(["--object", "1"])
    capsys.readouterr()
    assert tools.main(["object-irt", d, "--object", "1"]) == 1 and "not overwritten" in capsys.readouterr().out
    os.remove(dst)
    base = str(tmp_path / "other.hdr")
    IO.write_hdr(base, E * F32(2))
    rc, got, _ = run(["--object", "1", "--base", base])
    IO.write_hdr(ref, np.maximum(np.asarray(IO.read_hdr(base), F32) - rd("0_irr_texture_object1_shadow.hdr"), F32(0)))
    assert rc == 0 and got == open(ref, "rb").read()
