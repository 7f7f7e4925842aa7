"""CPU: the float64 reference of the inserted lights' specular rule (spec_light_cases) is sharp enough to bind, accepts the float32 restatement of the
header's sequence and rejects the ways the pass can go wrong; the rule itself converges to the integral it estimates; the C-ABI, Scene.spec_lights and
irtlight.add_view exist; the evaluation model without test.lights draws and returns what it did before.

  * caps, from the reference alone, on every case: no overflowing candidate list, at most 1 % of the live terms uncertain, at most 2 % of the pixels
    holding one;
  * spec_lights_f32 lies inside every interval of every case; each mutant falls out on its named case (terms added in the other order: other bits);
  * convergence per roughness, float64, nothing in the way: the balance estimate at S = 4096 against the midpoint rule over the light's area at 2^18
    cells; the margin is CONVERGENCE_FACTOR times that estimate's own change from 2^17 to 2^18 cells plus the balance estimate's own standard error over
    seeded shifts (spec_light_cases: CONVERGENCE).
"""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import spec_light_cases as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F32 = {}


def restated(name):
    if name not in _F32:
        _F32[name] = SL.spec_lights_f32(SL.case(name))
    return _F32[name]


@pytest.mark.parametrize("name", SL.ALL)
def test_caps_and_the_float32_restatement(name):
    c = SL.case(name)
    ref = c.ref()
    over, us, ut = ref.caps()
    print("spec light case %-16s %s" % (name, json.dumps(ref.summary())))
    assert over == 0 and us <= SL.CAP_UNCERTAIN_TERMS and ut <= SL.CAP_UNCERTAIN_PIXELS
    R, stats = restated(name)
    fails, worst = SL.check(c, R, stats, SL.SENTINEL)
    print("spec_lights_f32 %-16s worst share of an interval %.3f, stats %s inside %s" % (name, worst, stats.tolist(), ref.counts()))
    assert not fails, fails
    if name == "empty":
        assert (R == SL.SENTINEL).all() and not stats.any()
    if name == "room_eight":
        assert not R[[1, 3, 4, 5, 6]][:, ref.tex].any() and all((R[k][ref.tex] > 0).any() for k in (0, 2, 7))
    if name == "on_wall":
        assert stats[1] == stats[0] > 0
    if name == "box_special":
        row = lambda nm: [4 * c.names.index(nm) + j for j in range(4)]
        for nm in ("light_behind_surface", "zero_normal"):
            assert not R[:, row(nm)].any(), nm
        assert not R[1, row("inside_sphere")].any()
        for nm in ("mirror_sphere", "mirror_quad", "light_behind_camera", "scaled_normal", "tilted_normal", "wall"):
            assert (R[:, row(nm)] > 0).any(), nm
        assert ref.traced_yes[0, 1].sum() > 10 and ref.traced_yes[1, 1].sum() > 4             # live lobe terms on both lights
    if name == "box_lobe":                                                      # the lobe technique's case
        assert ref.traced_yes[0, 1].sum() > 400 and ref.traced_yes[0, 0].sum() > 2000


@pytest.mark.parametrize("mut", SL.MUTANTS)
def test_mutants_are_rejected(mut):
    c = SL.case(SL.MUTANT_CASES[mut])
    base = restated(c.name)
    assert not SL.check(c, *base)[0]
    R, stats = SL.spec_lights_f32(c, mut)
    if mut == "order_swapped":                                                  # the other order is as good an estimate: only the bits tell
        assert not np.array_equal(R.view(np.uint32), base[0].view(np.uint32))
        return
    fails, _ = SL.check(c, R, stats)
    assert fails, "mutant %s was accepted on %s" % (mut, c.name)
    print("mutant %-16s on %-16s: %s" % (mut, c.name, fails[0]))


def test_the_checker_sees_writes_outside_the_list_and_bad_stats():
    c = SL.case("list65")
    R, stats = restated("list65")
    G = R.copy()
    G[0, np.setdiff1d(np.arange(c.P), c.ref().tex)[3]] = 0.0
    assert SL.check(c, G, stats, SL.SENTINEL)[0]
    assert SL.check(c, R, stats + np.array([0, 5]), SL.SENTINEL)[0] or SL.check(c, R, stats - np.array([0, 5]), SL.SENTINEL)[0]


@pytest.mark.parametrize("r", SL.ROUGHNESS)
def test_the_rule_converges_to_the_area_integral(r):
    x, n, rr, cam, recs = SL.convergence_case(r)
    shifts = np.random.default_rng(61).random((SL.CONVERGENCE_SHIFTS, 2), dtype=np.float32)
    for rec in recs:
        a17, a18 = SL.area_estimate(x, n, rr, cam, rec, (256, 512)), SL.area_estimate(x, n, rr, cam, rec, (512, 512))
        b = np.array([SL.balance_estimate(x, n, rr, cam, sh, rec, 4096) for sh in shifts])
        se = b.std(ddof=1) / np.sqrt(len(b))
        margin = SL.CONVERGENCE_FACTOR * abs(a18 - a17) + SL.CONVERGENCE_SIGMAS * se
        dev = abs(b.mean() - a18)
        print("r = %-4g %-6s area 2^18 %.9g (change from 2^17 %.3e), balance S = 4096 mean of %d shifts %.9g (standard error %.3e): deviation %.3e = %.3f of the margin"
              % (r, "quad" if rec[0] == 0 else "sphere", a18, abs(a18 - a17), len(b), b.mean(), se, dev, dev / margin))
        assert a18 > 0 and dev <= margin and margin <= 0.05 * a18, "the margin itself must stay sharp: 5 % of the value"


# ---- the C-ABI and the Python surface (fails on the parent commit) ---------------------------------------------------------------------------------------------------

def test_header_declares_and_the_loader_binds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    from texir_code_amd import _lib, irtlight, scene
    for name in ("texir_spec_lights", "texir_spec_lights_any"):
        m = re.search(r"TEXIR_API int %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared" % name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == 17 and len(_lib.signatures()[name]) == n_args
    text = hdr[hdr.index("the SPECULAR response to new area lights"):hdr.index("TEXIR_API int texir_spec_lights(")]
    for word in ("FLOAT32 OPERATION SEQUENCE", "ROUNDING BOUND", "LIGHT SAMPLE", "LOBE SAMPLE", "pL", "pB", "t_max", "clamp_eps"):
        assert word in text, word
    mk = open(os.path.join(ROOT, "texir_code_amd", "csrc", "Makefile")).read()
    assert mk.count("speclight.hip") == 2
    assert callable(scene.Scene.spec_lights) and callable(irtlight.add_view)


def test_add_view_is_the_written_formula_in_numpy_and_torch():
    from texir_code_amd import irtlight
    rng = np.random.default_rng(5)
    rgb, alb = rng.random((6, 5, 3), dtype=np.float32), rng.random((6, 5, 3), dtype=np.float32)
    F, R = rng.random((2, 6, 5), dtype=np.float32), rng.random((2, 6, 5), dtype=np.float32)
    cols = [(2.0, 1.0, 0.5), 3.0]
    pi = np.float32(np.pi)
    want = rgb
    for k in range(2):
        want = want + (alb / pi * F[k][..., None] + R[k][..., None]) * np.asarray(cols[k], np.float32).reshape(-1)
    got = irtlight.add_view(rgb, alb, F, R, cols)
    assert got.dtype == np.float32 and np.array_equal(got, want) and (got != rgb).any()
    gt = irtlight.add_view(*(torch.from_numpy(a) for a in (rgb, alb, F, R)), cols)
    assert torch.is_tensor(gt) and np.array_equal(gt.numpy(), want)
    assert np.array_equal(irtlight.add_view(rgb, alb, F[:0], R[:0], []), rgb)
    for bad in (lambda: irtlight.add_view(rgb, alb, F, R, cols[:1]), lambda: irtlight.add_view(rgb, alb, F, R[:1], cols),
                lambda: irtlight.add_view(rgb, alb[:5], F, R, cols), lambda: irtlight.add_view(rgb, alb, F[:, :5], R[:, :5], cols)):
        with pytest.raises(ValueError):
            bad()


# ---- the evaluation model without test.lights: the same draws, the same bits -------------------------------------------------------------------------------------------

class _NoScene:
    """render() without lights must not ask the scene for anything but what spec_render (replaced below) takes"""

    def __getattr__(self, name):
        raise AssertionError("render() touched scene.%s without test.lights" % name)


def _model(monkeypatch, relighting=False):
    """the model the tester runners get (plugin registry), on the CPU: the base module's two GPU calls replaced by plain torch functions"""
    from texir_code_amd import plugin
    from texir_code_amd.tester import lit_model as LM, test_model as TM
    assert plugin.get_class("models.test_nvdiffrast.MaterialModel") is LM.MaterialModel and issubclass(LM.MaterialModel, TM.MaterialModel)
    calls = []

    def fake_spec_render(scene, normal, albedo, roughness, points, irr, cam, shift, S, clamp_eps):
        calls.append(("spec", S, clamp_eps))
        return irr * albedo + shift.sum(1, keepdim=True) * roughness[:, None] + normal * points

    def fake_diffuse(scene, points, normal, shift, N, mode):
        calls.append(("diffuse", N, mode))
        return points + shift[:, :1]
    monkeypatch.setattr(TM, "spec_render", fake_spec_render)
    monkeypatch.setattr(TM, "diffuse_irradiance", fake_diffuse)
    m = LM.MaterialModel.__new__(LM.MaterialModel)
    torch.nn.Module.__init__(m)
    m.scene, m.device, m.sample_l, m.sample_type, m.relighting = _NoScene(), torch.device("cpu"), [8, 16], ["uniform", "importance"], relighting
    return LM, TM, m, calls, fake_spec_render, fake_diffuse


def _parent_render(TM, spec, diffuse, relighting, normal, albedo, rough, points, cam, irr, P):
    """the render of the base class restated: one draw of [P,1,2] per traced term, the diffuse term's first"""
    n_, a_, r_, p_, i_ = normal.reshape(P, 3), albedo.reshape(P, 3), rough.reshape(P), points.reshape(P, 3), irr.reshape(P, 3)
    if relighting:
        i_ = diffuse(None, p_, n_, torch.rand(P, 1, 2).reshape(P, 2), 8, "uniform")
    shift = torch.rand(P, 1, 2).reshape(P, 2)
    return spec(None, n_, a_, r_, p_, i_, cam, shift, 16, TM.TINY_NUMBER), shift


@pytest.mark.parametrize("relighting", [False, True])
def test_evaluation_render_without_lights_draws_and_returns_what_it_did(monkeypatch, relighting):
    LM, TM, m, calls, spec, diffuse = _model(monkeypatch, relighting)
    g = torch.Generator().manual_seed(3)
    shape = (6, 2, 3)
    P = 36
    normal, albedo, points, irr = (torch.rand(shape + (3,), generator=g) for _ in range(4))
    rough, cam = torch.rand(shape + (1,), generator=g), torch.tensor([0.3, 1.5, -0.2])
    torch.manual_seed(11)
    want = _parent_render(TM, spec, diffuse, relighting, normal, albedo, rough, points, cam, irr, P)[0].reshape(shape + (3,))
    state = torch.get_rng_state()
    del calls[:]
    base = TM.MaterialModel.__new__(TM.MaterialModel)                      # the base class itself: what every pull request before this one rendered
    torch.nn.Module.__init__(base)
    base.scene, base.device, base.sample_l, base.sample_type, base.relighting = m.scene, m.device, m.sample_l, m.sample_type, relighting
    for variant, model in (("base class", base), ("attribute absent", m), ("attribute None", m)):
        if variant == "attribute None":
            m.test_lights = None
        torch.manual_seed(11)
        res = model.render(normal, albedo, rough, points, cam, irr)
        assert torch.equal(res["rgb"], want), variant
        assert torch.equal(torch.get_rng_state(), state), "%s: render drew another number of generator values" % variant
        assert set(res) == {"rgb", "albedo", "normal", "position"}
    assert [c[0] for c in calls] == (["diffuse", "spec"] if relighting else ["spec"]) * 3
    assert LM.load_test_lights("none", torch.device("cpu")) is None and LM.load_test_lights("None", torch.device("cpu")) is None


@pytest.mark.parametrize("relighting", [False, True])
def test_evaluation_render_with_lights_adds_add_view_and_draws_nothing_more(monkeypatch, tmp_path, relighting):
    from texir_code_amd import irtlight
    LM, TM, m, calls, spec, diffuse = _model(monkeypatch, relighting)
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [0, 2.5, 0], "a": [1, 0, 0], "b": [0, 0, 1], "colour": [10, 9, 8]}, {"kind": "sphere", "c": [1, 1, 1], "r": 0.25}]}))
    m.test_lights, m.light_samples = LM.load_test_lights(str(js), torch.device("cpu")), 32
    assert tuple(m.test_lights[0].shape) == (2, 16) and tuple(m.test_lights[1].shape) == (2, 3)
    seen = {}

    def irt_lights(pos, nrm, shift, lights, S):
        seen["F"] = (shift.clone(), S)
        return torch.stack([pos[:, 0] * 0.5, nrm[:, 1] + 1.0])

    def spec_lights(pos, nrm, rough, shift, cam, lights, S, clamp_eps):
        seen["R"] = (shift.clone(), S, clamp_eps)
        return torch.stack([rough * 2.0, pos[:, 2]])
    m.scene = types.SimpleNamespace(irt_lights=irt_lights, spec_lights=spec_lights)
    g = torch.Generator().manual_seed(4)
    normal, albedo, points, irr = (torch.rand((6, 2, 2, 3), generator=g) for _ in range(4))
    rough, cam = torch.rand((6, 2, 2, 1), generator=g), torch.tensor([0.3, 1.5, -0.2])
    torch.manual_seed(12)
    plain, shift = _parent_render(TM, spec, diffuse, relighting, normal, albedo, rough, points, cam, irr, 24)
    state = torch.get_rng_state()
    F, R = irt_lights(points.reshape(24, 3), normal.reshape(24, 3), shift, None, 32), spec_lights(points.reshape(24, 3), None, rough.reshape(24), shift, cam, None, 32, 0)
    want = irtlight.add_view(plain, albedo.reshape(24, 3), F, R, m.test_lights[1])
    torch.manual_seed(12)
    res = m.render(normal, albedo, rough, points, cam, irr)
    assert torch.equal(res["rgb"], want.reshape(6, 2, 2, 3)) and not torch.equal(want, plain)
    assert torch.equal(torch.get_rng_state(), state), "the lights drew from the CPU generator"
    # the pixels' own SPECULAR shift (with relighting: the second draw), the same for both passes
    assert torch.equal(seen["F"][0], shift) and torch.equal(seen["R"][0], shift) and seen["F"][1] == seen["R"][1] == 32 and seen["R"][2] == TM.TINY_NUMBER
