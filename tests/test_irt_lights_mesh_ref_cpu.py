"""The reference of the inserted lights behind inserted mesh objects (tests/light_mesh_cases.py; include/texir_hip.h texir_irt_lights_mesh,
texir_spec_lights_mesh) checked against itself, no device: the caps per case, the float32 restatement inside the float64 reference, every mutant rejected on
its case, the identities with the object-free rule, the prefilter, the conf keys and the tool."""
import os

import numpy as np
import pytest

import light_cases as LC
import light_mesh_cases as LM
import spec_light_cases as SL

F32 = np.float32
_F32 = {}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def restated(name):
    if name not in _F32:
        _F32[name] = LM.lights_mesh_f32(LM.case(name))
    return _F32[name]


# ---- the reference's own caps, the restatement inside it ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LM.ALL)
def test_caps_and_the_restatement_inside_the_reference(name):
    c = LM.case(name)
    r = c.ref()
    over, share_samples, share_texels = r.caps()
    print("irt_lights_mesh %s: %s; samples certainly blocked by an object alone: %d" % (name, r.summary(), int(r.blocked_by_object.sum())))
    assert over == 0 and share_samples <= LM.CAP_UNCERTAIN_SAMPLES and share_texels <= LM.CAP_UNCERTAIN_TEXELS
    F, st = restated(name)
    fails, worst = LM.check(c, F, st, LM.SENTINEL)
    assert not fails, "\n".join(fails)
    if c.J and name not in ("below", "nonfinite"):
        assert r.blocked_by_object.any(), "the case's objects block nothing: it checks nothing new"


@pytest.mark.parametrize("name", LM.SPEC_ALL)
def test_specular_caps_and_the_restatement_inside_the_reference(name):
    c = LM.spec_case(name)
    r = c.ref()
    over, share_terms, share_pixels = r.caps()
    print("spec_lights_mesh %s: %s" % (name, r.summary()))
    assert over == 0 and share_terms <= SL.CAP_UNCERTAIN_TERMS and share_pixels <= SL.CAP_UNCERTAIN_PIXELS
    R, st = LM.spec_lights_mesh_f32(c)
    fails, worst = LM.check(c, R, st, LM.SENTINEL)
    assert not fails, "\n".join(fails)
    # the objects matter: the object-free restatement is not accepted (dup_outside's triangle shadows a few of its 40 pixels only)
    if name != "dup_outside":
        R0, st0 = SL.spec_lights_f32(c.base)
        assert LM.check(c, R0, st0, LM.SENTINEL)[0], "the reference accepts the result without objects"


@pytest.mark.parametrize("mut", LM.MUTANTS)
def test_every_mutant_is_rejected_on_its_case(mut):
    c = LM.case(LM.MUTANT_CASES[mut])
    F, st = LM.lights_mesh_f32(c, mut)
    fails, _ = LM.check(c, F, st, LM.SENTINEL)
    assert fails, "the check accepts the mutant %s on %s" % (mut, c.name)
    assert not LM.check(c, *restated(LM.MUTANT_CASES[mut]), LM.SENTINEL)[0]


# ---- identities -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("none", "below", "nonfinite"))
def test_objects_that_block_nothing_reproduce_the_object_free_bits(name):
    c = LM.case(name)
    F, st = restated(name)
    F0, st0 = LC.lights_f32(c.base)
    assert np.array_equal(bits(F), bits(F0)) and st.tolist() == st0.tolist()


@pytest.mark.parametrize("name", ("tri", "cube", "twice", "one_sample", "behind_light", "enclosed", "inside_box"))
def test_the_prefilter_changes_no_bit_of_the_restatement(name):
    c = LM.case(name)
    F, st = restated(name)
    F1, st1 = LM.lights_mesh_f32(c, prefilter=False)
    assert np.array_equal(bits(F), bits(F1)) and st.tolist() == st1.tolist()


def test_monotone_and_zero_in_the_restatement():
    for name in ("tri", "cube", "twice", "inside_box"):
        c = LM.case(name)
        F, _ = restated(name)
        F0, _ = LC.lights_f32(c.base)
        rows = c.ref().tex
        assert (F[:, rows] <= F0[:, rows]).all(), name
    c = LM.case("enclosed")
    F, st = restated("enclosed")
    assert not bits(F[:, c.ref().tex]).any() and st[0] > 0 and st[1] == 0
    c = LM.case("inside_box")
    F, _ = restated("inside_box")
    assert not bits(F[0, c.ref().tex]).any() and (F[1, c.ref().tex] > 0).any()      # the panel is shut out, the sphere inside the box is seen


# ---- conf keys ------------------------------------------------------------------------------------------------------------------------------------------------------

class _Conf(dict):
    def get(self, k, d=None):
        return dict.get(self, k, d)


def test_conf_keys_parse_and_bad_values_raise(tmp_path):
    from texir_code_amd import irtobject, models
    from texir_code_amd.conf import ConfigFactory
    from texir_code_amd.tester import lit_model as LIT
    objs = irtobject.parse([{"obj": "table.obj"}])
    assert models.irt_light_objects_setting(_Conf(), "none", None) is False
    assert models.irt_light_objects_setting(_Conf({"train.irt_light_objects": False}), "none", None) is False
    p = tmp_path / "a.conf"
    p.write_text("train {\n    irt_light_objects = true\n}\n")
    conf = ConfigFactory.parse_file(str(p))
    assert models.irt_light_objects_setting(conf, "lights.json", objs) is True
    for lights, objects in (("none", objs), ("lights.json", None), ("none", None)):
        with pytest.raises(ValueError, match="train.irt_light_objects = true needs train.irt_lights .* and train.irt_objects"):
            models.irt_light_objects_setting(conf, lights, objects)
    for bad in ("yes", 1, 0.5, None):
        with pytest.raises(ValueError, match="train.irt_light_objects must be true or false"):
            models.irt_light_objects_setting(_Conf({"train.irt_light_objects": bad}), "lights.json", objs)
    # test.objects
    assert LIT.load_test_objects("none", None, "cpu") is None and LIT.load_test_objects("None", (1, 2), "cpu") is None
    with pytest.raises(ValueError, match="test.objects needs test.lights"):
        LIT.load_test_objects([{"obj": "table.obj"}], None, "cpu")
    with pytest.raises(ValueError, match="test.objects must be none, a list"):
        LIT.load_test_objects(7, (1, 2), "cpu")
    with pytest.raises(ValueError, match="test.objects: entry 0 must be"):
        LIT.load_test_objects([{"pose": None}], (1, 2), "cpu")
    with pytest.raises(FileNotFoundError, match="test.objects = .*nowhere.json"):
        LIT.load_test_objects(str(tmp_path / "nowhere.json"), (1, 2), "cpu")
    with pytest.raises(FileNotFoundError, match="no such file"):
        LIT.load_test_objects([{"obj": str(tmp_path / "missing.obj")}], (1, 2), "cpu")


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_light_irt_objects_takes_the_object_files_and_names_what_is_missing(tmp_path, capsys):
    from texir_code_amd import io_formats as IO, irtlight, tools
    rng = np.random.default_rng(12)
    d = str(tmp_path)
    E = rng.random((8, 8, 3), dtype=F32) + F32(0.5)
    IO.write_hdr(os.path.join(d, "0_irr_texture.hdr"), E)
    rd = lambda n: np.asarray(IO.read_hdr(os.path.join(d, n)), F32)
    plainF = rng.random((2, 8, 8), dtype=F32)
    for k in range(2):
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d.hdr" % k), np.repeat(plainF[k][..., None], 3, -1))
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d_bounce.hdr" % k), rng.random((8, 8, 3), dtype=F32))
    both = ["light-irt", d, "--light", "0", "--colour", "2,2,2", "--light", "1", "--colour", "1,0.5,3"]
    cols = [(2.0, 2.0, 2.0), (1.0, 0.5, 3.0)]
    lit = os.path.join(d, "0_irr_texture_lit.hdr")

    def run(argv):
        if os.path.exists(lit):
            os.remove(lit)
        rc = tools.main(argv)
        return rc, (open(lit, "rb").read() if rc == 0 else None)
    rc, plain = run(both)
    assert rc == 0
    capsys.readouterr()
    assert run(both + ["--objects"])[0] == 1                                      # no object files yet: the file and the conf key are named
    msg = capsys.readouterr().out
    assert "0_irr_texture_light0_objects.hdr" in msg and "train.irt_light_objects" in msg
    objF = (plainF * rng.random((2, 8, 8), dtype=F32)).astype(F32)
    for k in range(2):
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d_objects.hdr" % k), np.repeat(objF[k][..., None], 3, -1))
    E = rd("0_irr_texture.hdr")
    F = np.stack([rd("0_irr_texture_light%d_objects.hdr" % k)[..., 0] for k in range(2)])
    ref = str(tmp_path / "ref.hdr")
    rc, got = run(both + ["--objects"])
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add(E, F, cols), F32))
    assert rc == 0 and got == open(ref, "rb").read() and got != plain
    assert run(both)[1] == plain                                                  # without the flag: the file it wrote before
    capsys.readouterr()
    assert run(both + ["--objects", "--bounce"])[0] == 1
    msg = capsys.readouterr().out
    assert "0_irr_texture_light0_objects_bounce.hdr" in msg and "train.irt_light_objects" in msg and "train.irt_light_bounces" in msg
    for k in range(2):
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d_objects_bounce.hdr" % k), rng.random((8, 8, 3), dtype=F32) * F32(0.25))
    G = np.stack([rd("0_irr_texture_light%d_objects_bounce.hdr" % k) for k in range(2)])
    rc, got = run(both + ["--bounce", "--objects"])
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add_indirect(irtlight.add(E, F, cols), G, cols), F32))
    assert rc == 0 and got == open(ref, "rb").read()
    # the full relit atlas: the objects' shadow on the captured light as the base
    base = os.path.join(d, "0_irr_texture_objects.hdr")
    IO.write_hdr(base, (E * F32(0.5)).astype(F32))
    rc, got = run(both + ["--objects", "--base", base])
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add(rd("0_irr_texture_objects.hdr"), F, cols), F32))
    assert rc == 0 and got == open(ref, "rb").read()
    assert tools.main(["light-irt", d, "--objects=1", "--light", "0", "--colour", "1,1,1"]) == 2
