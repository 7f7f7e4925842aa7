"""CPU: the reference of the specular shadow pass (spec_shadow_cases) is sharp and sound before any GPU runs -- every case inside its caps, a float32
restatement of the rule inside its bounds, the eleven mutants it must reject -- and the layers above the kernel that need no device: the header's
declaration, the ctypes signature, the Makefile entry, the C-ABI's refusals, add_view(lost_spec=), the conf key, the sets of Scene.spec_shadow."""
import ctypes as Ct
import os
import re

import numpy as np
import pytest

import spec_cases as SC
import spec_shadow_cases as C

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1                # TEXIR_ERR_INVALID
D = 8                       # a dummy non-null pointer


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.CPU_CASES)
def test_every_case_stays_inside_its_caps(name):
    r = C.case(name).ref()
    over, left, multi, unc = r.caps()
    print(name, "caps", r.caps(), "counts", r.counts())
    assert over == 0, "%d rays overflow a candidate list" % over
    assert left <= C.CAP_LEFT_OUT, "%.5f of the samples have more than %d uncertain kinks" % (left, SC.MAX_UNC)
    assert multi <= C.CAP_MULTI, "%.4f of the rays that may meet something have several candidate hits" % multi
    assert unc <= C.CAP_UNCERTAIN_PIXELS, "%.4f of the listed pixels have an uncertain blocked decision" % unc


def test_the_cases_cover_what_the_issue_lists():
    names = C.GPU_CASES
    shape = {n: (int(n[1:].split("_p")[0]), int(n.split("_p")[1])) for n in names if re.fullmatch(r"s\d+_p\d+", n)}
    assert {(1, p) for p in (1, 63, 64, 65, 200)} | {(16, p) for p in (3, 4, 5)} | {(64, 1), (64, 2)} <= set(shape.values())
    cs = {n: C.case(n) for n in C.CPU_CASES}
    for n, (S, P) in shape.items():
        if n in cs:
            assert cs[n].S == S and len(cs[n].ids) == P
    g = C.case("s16_grid")
    assert len(g.ids) == 4 * 3 * 8 + 7 and g.grid_cap == 2 and g.S == 16
    assert {c.S for c in cs.values()} >= {1, 16, 24, 64, 100}
    assert set(C.LPP_CASES) == {"lpp%d_s%d" % (l, s) for l in (1, 4, 16) for s in (16, 24)} and cs["lpp4_s24"].lpp == 4
    every = [C.case(n) for n in ("s1_p1", "s1_p63", "s1_p64", "s1_p65", "s1_p200", "s16_p5")]
    assert {c.M for c in every} == {1, 2, 3, 4, 5, 8}
    assert {(0, 0), (1, 0), (0, 1), (8, 8), (3, 2)} <= {(c.Kb, c.J) for c in list(cs.values()) + [C.case("s64_p1")]}
    assert len(cs["twice"].occ) == 1 and cs["twice"].J == 2, "an instance named twice"
    assert not np.isfinite(cs["nan_matrix"].w2o).all(), "a matrix with a NaN"
    from light_cases import record_kind
    assert [record_kind(r) for r in cs["s24_eight"].bodies].count(None) == 2, "invalid body records"
    assert tuple(C.ROUGHNESS) == (0.01, 0.1, 0.5, 0.8) and set(np.unique(cs["s100"].rough).tolist()) <= set(np.asarray(C.ROUGHNESS, F32).tolist())
    assert {"tri", "cube", "ico", "table"} <= {n for c in cs.values() for n in c.occ} and "person" in C.case("room_person").occ
    assert {"tri", "cube", "ico", "table", "person"} <= {n for name in C.GPU_CASES for n in C.case(name).occ}
    grid = C.case("s16_grid").ref()
    assert 0 < grid.uncertain.any(1).sum() <= C.CAP_UNCERTAIN_PIXELS * len(grid.pix), "a case whose reference leaves some blocked decisions open, under the cap"


def test_the_named_geometries_do_what_their_names_say():
    far, none, top = C.case("far").ref(), C.case("none").ref(), C.case("open_top").ref()
    assert far.meet_yes.sum() > 0 and far.blk_maybe.sum() == 0 and not any(np.abs(m).any() for m in far.mid), "met, never in front of an accepted hit"
    assert none.meet_maybe.sum() == 0
    assert top.meet_yes.sum() > 0 and top.blk_maybe.sum() == 0, "the body above the open top is met only by rays that leave the scene"
    for n in ("in_ball", "in_cube"):
        r = C.case(n).ref()
        assert r.all_blocked(0).all() and len(r.pix) >= 12, n
    ov = C.case("overlap").ref()
    assert np.abs(ov.mid[1]).any() and np.abs(ov.mid[2]).any() and (ov.mid[0] >= ov.mid[1]).all()
    hb = C.case("highbits")
    assert hb.masks() == [0x101, 0x000, 0x000] and len(hb.buf) == 2 and len(hb.inst_buf) == 2


@pytest.mark.parametrize("name", C.CPU_CASES)
def test_float32_restatement_lies_inside_the_reference(name):
    c = C.case(name)
    lost, stats = C.spec_shadow_f32(c)
    assert C.check(c, lost, stats, C.SENTINEL, "float32 restatement") <= 1.0
    # the prefilter changes no bit of the restatement (and spec_shadow_f32 asserts that it rejects no ray the leaf test accepts)
    off, st_off = C.spec_shadow_f32(c, prefilter=False)
    assert np.array_equal(lost.view(np.uint32), off.view(np.uint32)) and st_off[2] == stats[2]


@pytest.mark.parametrize("mut", C.MUTANTS)
def test_the_check_rejects_the_mutant(mut):
    c = C.case(C.MUTANT_CASES[mut])
    C.check(c, *C.spec_shadow_f32(c), C.SENTINEL, "unmutated")
    lost, stats = C.spec_shadow_f32(c, mut)
    assert C.rejected(C.check, c, lost, None, C.SENTINEL, mut), "the mutant %s passes on %s" % (mut, c.name)


def test_the_mutant_list_is_the_documented_one():
    assert C.MUTANTS == ("far_ignored", "one_sided", "shell", "sum_sets", "inst_bits_low", "high_bits", "no_weight", "ndl_weight", "no_over_S", "world_space",
                         "add_missed") and set(C.MUTANT_CASES) == set(C.MUTANTS)


def test_where_every_sample_is_blocked_the_restatement_is_the_specular_term_bit_for_bit():
    """the header's first consequence on the restatement: inside the ball, lost is the whole specular sum -- the same terms in the same order"""
    c = C.case("in_ball")
    lost, _ = C.spec_shadow_f32(c)
    w, l = C.chain_f32(c)
    t, pid, rad = C._TRACED[c.name]
    P, S = len(c.listed), c.S
    acc = np.isfinite(t) & (t > F32(1e-4)) & (pid >= 0)
    Lr = np.where(acc[:, None], rad, F32(0)).astype(F32)
    whole = (C.reduce_f32((Lr.reshape(P, S, 3), w.reshape(P, S)), np.ones((P, S), bool), S, SC.lanes_per_pixel(S)) / F32(S)).astype(F32)
    assert np.array_equal(lost[0][c.listed].view(np.uint32), whole.view(np.uint32)) and (whole > 0).any()


# ---- the layers above the kernel -------------------------------------------------------------------------------------------------------------------------------

def test_header_ctypes_and_makefile_carry_the_entry_point():
    from texir_code_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    m = re.search(r"TEXIR_API int texir_spec_shadow\((.*?)\);", hdr, re.S)
    assert m, "the header does not declare texir_spec_shadow"
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    sig = _lib.signatures()["texir_spec_shadow"]
    assert len(args) == len(sig) == 24
    names = list(_lib.signatures())
    assert names.index("texir_spec_shadow") == names.index("texir_spec_lights_mesh") + 1, "the header's order"
    assert hdr.index("texir_spec_lights_mesh(") < hdr.index("texir_spec_shadow(") < hdr.index("texir_png_unfilter(")
    for text in ("Bit k (0..7) = body k".lower(), "bit 8 + j = instance j", "union, not", "Not computed", "spec_kernel<false, 4>", "TEXIR_SPEC_LPP"):
        assert text.lower() in hdr[hdr.index("csrc/specshadow.hip"):hdr.index("TEXIR_API int texir_spec_shadow(")].lower(), text
    mk = open(os.path.join(ROOT, "texir_code_amd", "csrc", "Makefile")).read()
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS")][0]
    loop = [l for l in mk.splitlines() if "kernel-resource-usage" in l][0]
    assert "specshadow.hip" in srcs and "specshadow.hip" in loop
    assert os.path.exists(os.path.join(ROOT, "texir_code_amd", "csrc", "specshadow.hip"))
    k = open(os.path.join(ROOT, "texir_code_amd", "csrc", "kernels.h")).read()
    assert "launch_spec_shadow(" in k


@pytest.fixture(scope="module")
def L():
    from texir_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


_HANDLES = (Ct.c_void_p * 8)(*([D] * 8))
_INST = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32)
ORDER = ("scene", "normal", "rough", "points", "cam", "shift", "ids", "n_ids", "P", "S", "ceps", "bodies", "Kb", "occ", "Q", "inst", "w2o", "J", "sets", "M", "flags",
         "out", "stats", "stream")


def shadow_args(**kw):
    a = dict(scene=D, normal=D, rough=D, points=D, cam=D, shift=D, ids=D, n_ids=64, P=100, S=16, ceps=1e-14, bodies=D, Kb=2, occ=Ct.cast(_HANDLES, Ct.c_void_p), Q=2,
             inst=_INST.ctypes.data_as(Ct.c_void_p), w2o=D, J=2, sets=D, M=3, flags=0, out=D, stats=None, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ORDER)


def refused(L, msg, **kw):
    rc = L.texir_spec_shadow(*shadow_args(**kw))
    got = L.texir_last_error().decode()
    assert rc == INVALID and got.startswith("texir_spec_shadow: " + msg), (kw, rc, got)


def test_cabi_refusals(L):
    none = dict(bodies=None, occ=None, inst=None, w2o=None, sets=None, out=None)  # the ranges are reported before any null buffer is touched
    refused(L, "Kb must be in 0..8, got 9", Kb=9, **none)
    refused(L, "Kb must be in 0..8, got -1", Kb=-1)
    refused(L, "Q must be in 0..8, got 9", Q=9, **none)
    refused(L, "J must be in 0..8, got 9", J=9, **none)
    refused(L, "J must be in 0..8, got -2", J=-2)
    refused(L, "M must be in 1..8, got 0", M=0, **dict(none, inst=_INST.ctypes.data_as(Ct.c_void_p), occ=Ct.cast(_HANDLES, Ct.c_void_p)))
    refused(L, "M must be in 1..8, got 9", M=9)
    refused(L, "inst_obj is null", inst=None)
    refused(L, "inst_obj[1] = 1 names no occluder (Q = 1)", Q=1, bodies=None, w2o=None, sets=None, out=None)
    bad = np.array([0, -1], np.int32)
    refused(L, "inst_obj[1] = -1 names no occluder (Q = 2)", inst=bad.ctypes.data_as(Ct.c_void_p))
    refused(L, "S must be in 1..65536, got 0", S=0, bodies=None, w2o=None, sets=None, out=None)
    refused(L, "S must be in 1..65536, got -3", S=-3)
    refused(L, "clamp_eps must be finite and > 0", ceps=0.0)
    refused(L, "negative pixel count", n_ids=-1)
    refused(L, "P too large", P=1 << 31)
    refused(L, "occluders is null", occ=None)
    holes = (Ct.c_void_p * 2)(D, None)
    refused(L, "occluders[1] is null", occ=Ct.cast(holes, Ct.c_void_p))
    refused(L, "bodies is null", bodies=None)
    refused(L, "sets is null", sets=None)
    for k in ("scene", "normal", "rough", "points", "cam", "shift", "out"):
        refused(L, "null argument", **{k: None})
    refused(L, "inst_world_to_obj is null", w2o=None)
    assert L.texir_spec_shadow(*shadow_args(n_ids=0, out=None)) == 0               # a non-null empty list writes nothing
    assert L.texir_spec_shadow(*shadow_args(Kb=0, bodies=None, J=0, Q=0, occ=None, inst=None, w2o=None, n_ids=0)) == 0


def test_add_view_takes_the_specular_shadow_first_and_none_changes_no_bit():
    import torch
    from texir_code_amd import irtlight
    rng = np.random.default_rng(4)
    shape = (5, 7, 3)
    rgb, alb, irr = (rng.random(shape, dtype=F32) for _ in range(3))
    F, R = rng.random((2,) + shape[:2], dtype=F32), rng.random((2,) + shape[:2], dtype=F32)
    G, lost = rng.random((2,) + shape, dtype=F32), rng.random(shape, dtype=F32) * F32(0.5)
    cols = [(2.0, 1.0, 0.5), (0.25, 0.5, 4.0)]
    ls = (rng.random(shape, dtype=F32) * F32(1.5)).astype(F32)                 # larger than rgb in places: the floor acts
    for kw in ({}, {"G": G}, {"lost": lost}, {"lost": lost, "irr": irr, "G": G}):
        old = irtlight.add_view(rgb, alb, F, R, cols, **kw)
        assert np.array_equal(old.view(np.uint32), irtlight.add_view(rgb, alb, F, R, cols, lost_spec=None, **kw).view(np.uint32)), "None: the bits of before"
        got = irtlight.add_view(rgb, alb, F, R, cols, lost_spec=ls, **kw)
        first = np.maximum(rgb - ls, F32(0))
        assert np.array_equal(got.view(np.uint32), irtlight.add_view(first, alb, F, R, cols, **kw).view(np.uint32)), "max(rgb - lost_spec, 0) is taken first"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        tk = {k: t(v) for k, v in kw.items()}
        assert np.array_equal(irtlight.add_view(t(rgb), t(alb), t(F), t(R), cols, lost_spec=t(ls), **tk).numpy().view(np.uint32),
                              irtlight.add_view(t(first), t(alb), t(F), t(R), cols, **tk).numpy().view(np.uint32)), "torch"
    assert (first == 0).any() and (first > 0).any()
    with pytest.raises(ValueError, match="lost_spec"):
        irtlight.add_view(rgb, alb, F, R, cols, lost_spec=ls[:4])


class _Conf(dict):
    def get(self, k, d=None):
        return dict.get(self, k, d)


def test_conf_key_parses_and_bad_values_raise(tmp_path):
    from texir_code_amd.conf import ConfigFactory
    from texir_code_amd.tester import lit_model as LM
    lights = (object(), object())
    assert LM.spec_shadow_setting(_Conf(), None) is False and LM.spec_shadow_setting(_Conf(), lights) is False
    for text, want in (("true", True), ("false", False)):
        p = tmp_path / ("%s.conf" % text)
        p.write_text("test {\n    spec_shadows = %s\n}\n" % text)
        assert LM.spec_shadow_setting(ConfigFactory.parse_file(str(p)), lights) is want
    assert LM.spec_shadow_setting(_Conf({"test.spec_shadows": False}), None) is False
    for bad in ("yes", 1, 0.5, None):
        with pytest.raises(ValueError, match="test.spec_shadows must be true or false"):
            LM.spec_shadow_setting(_Conf({"test.spec_shadows": bad}), lights)
    with pytest.raises(ValueError, match=r"test\.spec_shadows needs test\.lights"):
        LM.spec_shadow_setting(_Conf({"test.spec_shadows": True}), None)
    doc = LM.__doc__
    assert "test.spec_shadows" in doc and "Not computed" in doc and "shadow in the specular term of captured light" not in doc


def test_sets_of_spec_shadow():
    from texir_code_amd.scene import spec_shadow_sets as sets
    assert sets(None, 3, 2) == [0x307] and sets(None, 0, 0) == [0] and sets(None, 8, 8) == [0xFFFF]
    assert sets([5, 0, 0xFFFFFFFF, np.int64(0x100)], 1, 1) == [5, 0, 0xFFFFFFFF, 0x100], "an int mask is used as it is"
    assert sets([([0, 2], [1]), ([], []), ((1,), ())], 3, 2) == [0x205, 0, 2]
    assert sets([([0], [0]), 0x101], 1, 1) == [0x101, 0x101]
    for bad, text in (([([3], [])], "names body 3: the call has 3 bodies"), ([([-1], [])], "names body -1"), ([([], [2])], "names instance 2: the call has 2 instances"),
                      ([-1], "a mask is a uint32"), ([1 << 32], "a mask is a uint32"), (["01"], "an int mask or a pair"), ([(1, 2, 3)], "an int mask or a pair"),
                      ([True], "an int mask or a pair"), ([1.5], "an int mask or a pair")):
        with pytest.raises(ValueError, match=text):
            sets(bad, 3, 2)
