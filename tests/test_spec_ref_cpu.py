"""No GPU.  The float64 restatement of the GGX specular chain in tests/spec_cases.py is right (pinned against oracle/mat_step.spec_render in float64
with reverse-mode autograd -- an independent formulation -- and against the reference's goldens), and the bound and the kink variants that
test_gpu_spec_kernels.py relies on are neither too tight nor blind: legitimate float32 implementations pass the same checks on every case of the GPU
matrix with S <= 256, every operator mutant is rejected in the family built for it, and every case respects the caps (samples left out <= 0.1 %,
multi-variant samples of the smooth families <= 3 %, samples accepted only by a non-base variant <= 2 %) with the reference alone."""
import functools
import math

import numpy as np
import pytest
import torch

import spec_cases as SC
from conftest import rel_l2
from oracle import mat_step as MS

F32 = np.float32


@pytest.fixture(autouse=True)
def _threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, prev)))
    yield
    torch.set_num_threads(prev)


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def restated(c, dual=True, hooks=True):
    """the float64 restatement with e = 0 -> (w, dw, l) flat"""
    inp = c.inputs()
    if not dual:
        inp["r"].requires_grad_(True)
    ch = SC.Chain(inp, c.ceps, SC.Tape(on=hooks), dual=dual)
    w, l = ch.spec()
    dw = w.d if dual else torch.autograd.grad(w.v.sum(), inp["r"])[0]
    f = lambda x: x.detach().numpy()[:, 0]
    restated.edge_active = np.any([f(ch.kinks[k].nat) for k in ("s0_lo", "s0_hi", "s1_lo", "s1_hi", "ct_hi", "st_hi")], 0)
    return f(w.v), f(dw), np.stack([f(x.v) for x in l], -1)


@pytest.fixture
def float64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(prev)


# ---- pins ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ceps", [1e-14, 1e-6])
@pytest.mark.parametrize("S", [1, 16, 24])
def test_restatement_matches_float64_oracle_autograd(S, ceps, float64_default):
    """per-sample w and dw against oracle/mat_step.spec_render in float64 (reverse mode on the plain expression), observed through one-hot lighting;
    rgb, d_albedo, d_rough and l on random lighting.  Away from kinks, and away from the samples on which a clamp of s, ct or st is active: the
    oracle in float64 clamps at the float64 numbers 1e-6 and 1 - 1e-6, the reference (and the restatement) at their float32 roundings."""
    c = SC.smooth_case(40, S, seed=11, ceps=ceps)
    w, dw, l = restated(c)
    edge = restated.edge_active
    P = c.P
    rep = lambda x: t64(np.repeat(x, S, 0))
    r = rep(c.rough[:, None]).requires_grad_(True)
    L = torch.zeros(P * S, S, 3, dtype=torch.float64)
    L[torch.arange(P * S), torch.arange(S).repeat(P)] = 1.0
    rgb, _ = MS.spec_render(rep(c.normal), rep(c.albedo), r, rep(c.points), torch.zeros(P * S, 3, dtype=torch.float64), t64(c.cam), rep(c.shift), S, L,
                            ceps=float(F32(ceps)))
    w_o = rgb[:, 0] * S
    dw_o, = torch.autograd.grad(w_o.sum(), r)
    ref = c.ref()
    away = (ref.nunc == 0) & ~edge
    assert away.mean() > 0.9
    pix = ~edge.reshape(P, S).any(1)
    tol = lambda x: 1e-10 * np.abs(x) + 1e-13
    assert (np.abs(w - w_o.detach().numpy())[away] <= tol(w)[away]).all()
    assert (np.abs(dw - dw_o.numpy()[:, 0])[away] <= (tol(dw) + 1e-10 * np.abs(w))[away]).all()
    # per pixel, random lighting
    a, r = t64(c.albedo).requires_grad_(True), t64(c.rough[:, None]).requires_grad_(True)
    rgb, l_o = MS.spec_render(t64(c.normal), a, r, t64(c.points), t64(c.irr), t64(c.cam), t64(c.shift), S, t64(c.L), ceps=float(F32(ceps)))
    (rgb * t64(c.d_rgb)).sum().backward()
    assert np.abs(l.reshape(P, S, 3) - l_o.numpy())[pix].max() < 1e-12
    mine = c.diffuse() + (c.coef_rgb() * w.reshape(P, S, 1)).sum(1)
    assert (np.abs(mine - rgb.detach().numpy()) <= 1e-10 * np.abs(mine))[pix].all()
    assert np.abs(c.d_albedo()[0] - a.grad.numpy()).max() < 1e-12
    dr = (c.coef_drough() * dw.reshape(P, S, 1)).sum(1)
    scale = (np.abs(c.coef_drough()) * np.abs(dw).reshape(P, S, 1)).sum(1)
    assert (np.abs(dr - r.grad.numpy()) <= 1e-9 * scale + 1e-13)[pix].all()


@pytest.mark.parametrize("family", ["A", "B", "D"])
def test_dual_tangent_is_the_derivative(family):
    """the hooked dual-number pass (e = 0) against autograd of the plain restatement"""
    c = {"A": SC.smooth_case(60, 16, seed=12), "B": SC.roughness_cases(16)[5], "D": SC.view_cases(16)[2]}[family]
    w, dw, _ = restated(c)
    w2, dw2, _ = restated(c, dual=False, hooks=False)
    assert np.array_equal(w, w2)
    assert (np.abs(dw - dw2) <= 1e-10 * np.abs(dw2) + 1e-10 * np.abs(w) + 1e-13).all()


def test_float32_restatement_matches_goldens(golden):
    """tolerances of tests/test_mat_step_oracle.py"""
    g = golden("spec_render.npz")
    S = int(g["S"])
    c = SC.Case("golden", "G", g["normal"], g["roughness"], g["points"], g["cam"], g["shift"], S, 0)
    c.albedo, c.irr, c.L, c.d_rgb = g["albedo"], g["irr"], g["Ls"], g["d_rgb"]
    w, dw, l = SC.chain_f32(c)
    rgb, d_alb, d_r = SC.pixel_f32(c, w, dw)
    assert rel_l2(rgb, g["rgb"]) < 1e-6
    assert rel_l2(l.reshape(c.P, S, 3), g["l"]) < 1e-6
    assert rel_l2(d_alb, g["d_albedo"]) < 1e-6
    assert rel_l2(d_r, g["d_roughness"].reshape(-1)) < 1e-5
    # and the float64 restatement accepts the reference's own per-pixel numbers
    c.check_rgb(g["rgb"], "golden", "rgb")
    c.check_drough(g["d_roughness"], "golden", "d_rough")
    SC.check_exact(g["d_albedo"], *c.d_albedo(), "golden", "d_albedo")
    ref = SC.reference(c.inputs(), c.ceps, "spec", ("l0", "l1", "l2"))
    for k in range(3):
        SC.check_value(g["l"].reshape(-1, 3)[:, k], ref, "l%d" % k, "golden", "l component %d" % k)


def test_directions_match_gen_dir_golden(golden):
    """the reference's own float32 directions lie inside the bound of the float64 restatement, all three modes (no fixed tolerance: at r = 0.01 the
    reference's float32 direction is itself 4e-4 off)"""
    g = golden("gen_dir.npz")
    assert np.array_equal(g["normals"], SC.SPECIAL_NORMALS)
    for k in range(int(g["n_cases"])):
        mode, N = str(g["c%d_mode" % k]), int(g["c%d_N" % k])
        ref = SC.reference(SC.sample_inputs(g["normals"], g["roughness"], None, None, g["c%d_shift" % k], N), mode=mode, names=("d0", "d1", "d2"))
        L = g["c%d_L" % k].reshape(-1, 3)
        for a in range(3):
            SC.check_value(L[:, a], ref, "d%d" % a, "golden-dir", "%s N %d component %d" % (mode, N, a))


# ---- the matrix: float32 passes, caps hold -----------------------------------------------------------------------------------------------------------

def check_float32(c):
    ref = c.ref()
    assert np.isfinite(ref.val["w"][0]).all() and np.isfinite(ref.val["dw"][0]).all(), "%s: non-finite reference" % c.name
    assert ref.left.mean() <= SC.CAP_LEFT_OUT, "%s: %.5f of the samples left out" % (c.name, ref.left.mean())
    if c.smooth and ref.M >= 1000:
        assert ref.multi.mean() <= SC.CAP_MULTI_SMOOTH, "%s: %.4f of the samples multi-variant" % (c.name, ref.multi.mean())
    cap = SC.CAP_NONBASE
    fam = "cpu-" + c.family
    w, dw, l = SC.chain_f32(c)
    SC.check_value(w, ref, "w", fam, c.name + " w", named=c.named, cap=cap)
    SC.check_deriv(dw, ref, "dw", fam, c.name + " dw dual", named=c.named, cap=cap)
    _, dwa, _ = SC.chain_f32(c, dual=False)
    SC.check_deriv(dwa, ref, "dw", fam, c.name + " dw autograd", named=c.named, cap=cap)
    rgb, d_alb, d_r = SC.pixel_f32(c, w, dw)
    c.check_rgb(rgb, fam, c.name + " rgb")
    c.check_drough(d_r, fam, c.name + " d_rough")
    SC.check_exact(d_alb, *c.d_albedo(), fam, c.name + " d_albedo")
    # oracle/mat_step.spec_render in float32, per-pixel sums (torch's own summation order)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F32))
    a, r = t(c.albedo).requires_grad_(True), t(c.rough[:, None]).requires_grad_(True)
    rgb_o, _ = MS.spec_render(t(c.normal), a, r, t(c.points), t(c.irr), t(c.cam), t(c.shift), c.S, t(c.L), ceps=c.ceps)
    (rgb_o * t(c.d_rgb)).sum().backward()
    c.check_rgb(rgb_o.detach().numpy(), fam, c.name + " oracle f32 rgb")
    c.check_drough(r.grad.numpy(), fam, c.name + " oracle f32 d_rough")
    SC.check_exact(a.grad.numpy(), *c.d_albedo(), fam, c.name + " oracle f32 d_albedo")
    return ref


@pytest.mark.parametrize("S", [s for s in SC.S_LIST if s <= 256])
def test_float32_passes_and_caps_hold_on_shapes(S):
    multi = n = 0
    for c in SC.shape_cases(S):
        ref = check_float32(c)
        multi, n = multi + ref.multi.sum(), n + ref.M
    assert multi / n <= SC.CAP_MULTI_SMOOTH


def test_float32_passes_and_caps_hold_on_switch_shapes():
    """the inputs of the TEXIR_SPEC_GRID_CAP / TEXIR_SPEC_LPP / autograd cases of the GPU module"""
    cases = [SC.grid_cap_case(S, P) for S, P in SC.GRID_CAP_SHAPES] + [c for lpp, S in SC.LPP_SHAPES for c in SC.lpp_cases(lpp, S)] + [SC.autograd_case()]
    multi = n = 0
    for c in cases:
        ref = check_float32(c)
        multi, n = multi + ref.multi.sum(), n + ref.M
    assert multi / n <= SC.CAP_MULTI_SMOOTH


_FAMILY = SC.family_cases()


@pytest.mark.parametrize("c", _FAMILY, ids=[c.name for c in _FAMILY])
def test_float32_passes_and_caps_hold_on_families(c):
    check_float32(c)


def test_float32_directions_pass():
    for mode in ("uniform", "cosine", "importance"):
        rng = np.random.default_rng(3)
        n = np.concatenate([SC.frame_normals(), SC.unit_normals(40, rng)], 0)
        b = len(n)
        r, sh = rng.uniform(0, 1, b).astype(F32), rng.random((b, 2), F32)
        sh[::5] = 0
        for N in (1, 3, 64, 100):
            ref = SC.reference(SC.sample_inputs(n, r, None, None, sh, N), mode=mode, names=("d0", "d1", "d2"))
            assert ref.left.mean() <= SC.CAP_LEFT_OUT
            ch = SC.Chain(SC.sample_inputs(n, r, None, None, sh, N, torch.float32), 1e-14, SC.Tape(on=False), mode=mode)
            h = ch.direction()[2]
            for k in range(3):
                SC.check_value(h[k].v.double().numpy()[:, 0], ref, "d%d" % k, "cpu-dir", "%s N %d component %d" % (mode, N, k))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------------

def _axis_case():
    c = SC.smooth_case(40, 16, seed=13)
    n = c.normal.astype(np.float64)
    n[:, 0] = np.sign(n[:, 0] + 1e-9) * 0.95
    n[:, 1:] *= (math.sqrt(1 - 0.95 ** 2) / np.linalg.norm(n[:, 1:], axis=-1, keepdims=True))
    c.normal = np.ascontiguousarray(n, F32)
    c.points = SC.front_points(c.normal, np.random.default_rng(13))
    return c


@functools.lru_cache(None)
def _mutant_case(m):
    if m == "axis_09":
        return _axis_case()
    if m == "dots_unit_normal":
        return SC.frame_cases(16)[0]
    if m == "wrap_ge":
        return SC.shift_cases(16)[0]
    if m == "clamp_grad_outside":
        return SC.roughness_cases(16)[4]
    if m == "ceps_ignored":
        return SC.view_cases(16)[2]
    return SC.smooth_case(60, 16, seed=14)


@pytest.mark.parametrize("m", SC.MUTANTS)
def test_mutant_is_rejected(m):
    c = _mutant_case(m)
    ref = c.ref()
    w, dw, _ = SC.chain_f32(c)
    if m in ("dalbedo_no_pi", "inv_S_is_64"):
        rgb, d_alb, d_r = SC.pixel_f32(c, w, dw, mut=m)
        if m == "dalbedo_no_pi":
            assert SC.rejected(SC.check_exact, d_alb, *c.d_albedo(), "mutant")
        else:
            assert SC.rejected(c.check_rgb, rgb, "mutant") and SC.rejected(c.check_drough, d_r, "mutant")
        return
    # the unmutated float32 chain passes on the same case, the mutated one does not
    SC.check_value(w, ref, "w", "mutant-base")
    SC.check_deriv(dw, ref, "dw", "mutant-base")
    wm, dwm, _ = SC.chain_f32(c, mut=m)
    rej_w, rej_dw = SC.rejected(SC.check_value, wm, ref, "w", "mutant"), SC.rejected(SC.check_deriv, dwm, ref, "dw", "mutant")
    assert rej_dw if m in ("clamp_grad_outside", "ct_den_term_dropped") else rej_w, (m, rej_w, rej_dw)
    # ... and through the per-pixel sums as well
    rgb, _, d_r = SC.pixel_f32(c, wm, dwm)
    if m == "ct_den_term_dropped":
        assert SC.rejected(c.check_drough, d_r, "mutant")
    elif m != "clamp_grad_outside":              # (its family puts most samples on a kink: the per-pixel intervals are wide there, the per-sample check is the sharp one)
        assert SC.rejected(c.check_rgb, rgb, "mutant")
