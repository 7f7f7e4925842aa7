"""CPU: the reference of the body-shadow pass (irt_shadow_cases) is sharp and sound before any GPU runs -- its caps, a float32 restatement of the rule
inside its bounds on every case, the eight mutants it must reject, an analytic pin, the bit-identity geometry -- and the layers above the kernel that need
no device: the C-ABI's refusals, irtlight.add / add_view, the conf keys, the tool."""
import math
import os

import numpy as np
import pytest

import irt_shadow_cases as SH
import trace_cases as TC

F32 = np.float32
INVALID = -1                # TEXIR_ERR_INVALID
D = 8                       # a dummy non-null pointer


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SH.GPU_CASES)
def test_caps_of_every_case(name):
    r = SH.case(name).ref()
    over, unc = r.caps()
    print(name, r.summary())
    assert over == 0, "%d rays overflow their candidate list" % over
    assert unc <= SH.CAP_MULTI, "%.4f of the samples that may meet a body are uncertain" % unc


@pytest.mark.parametrize("name", SH.CPU_CASES)
def test_float32_restatement_lies_inside_the_reference(name):
    c = SH.case(name)
    lost, stats = SH.shadow_f32(c)
    worst = SH.check(c, lost, stats, SH.SENTINEL, "float32 restatement")
    assert worst <= 1.0
    s = c.ref().summary()
    if name not in ("box_nobody", "box_below"):
        assert s["may_meet"] > 0, "the case asks nothing"


@pytest.mark.parametrize("mut", SH.MUTANTS)
def test_the_check_rejects_the_mutant(mut):
    c = SH.case(SH.MUTANT_CASES[mut])
    SH.check(c, *SH.shadow_f32(c), SH.SENTINEL, "unmutated")
    lost, stats = SH.shadow_f32(c, mut)
    assert TC.rejected(SH.check, c, lost, stats, SH.SENTINEL, mut), "the mutant %s passes on %s" % (mut, c.name)


def test_the_mutant_list_is_the_documented_one():
    assert len(SH.MUTANTS) == 8 and set(SH.MUTANT_CASES) == set(SH.MUTANTS)


def test_body_rule_at_its_edges():
    """an exactly parallel ray, a quad met from either side, a point inside a ball, a ball behind the origin, refused records: the float32 rule and the
    float64 reference decide alike"""
    x = np.array([[0.0, 0.0, 0.0]], F32)
    q = SH.quad([-1.0, 1.0, -1.0], [2.0, 0.0, 0.0], [0.0, 0.0, 2.0])             # in the plane y = 1, a x b = (0, -4, 0)
    e0 = np.zeros((1, 3))

    def both(rec, d, fn):
        d = np.array([d], F32)
        m, t = fn(rec, x, d)
        B = SH.body64(x, d.astype(np.float64), e0, rec)
        assert bool(m[0]) == bool(B["meets"][0]) and (B["yes"][0] if m[0] else B["no"][0]), (d, m, B)
        return bool(m[0]), float(t[0])
    assert both(q, [1.0, 0.0, 0.0], SH.quad_f32) == (False, 0.0)                  # parallel: den == 0
    assert both(q, [0.0, 1.0, 0.0], SH.quad_f32) == (True, 1.0)                   # from the emitting side
    assert both(q, [0.0, -1.0, 0.0], SH.quad_f32) == (False, 0.0)                 # the plane lies behind the origin
    xa = np.array([[0.0, 2.0, 0.0]], F32)
    m, t = SH.quad_f32(q, xa, np.array([[0.0, -0.5, 0.0]], F32))                  # from its back, an un-normalised direction: t in units of |d|
    assert bool(m[0]) and float(t[0]) == 2.0
    assert both(q, [0.0, 1.0, 2.0], SH.quad_f32) == (False, 0.0)                  # the plane is met outside the parallelogram
    b = SH.ball([0.0, 0.25, 0.0], 1.0)
    assert both(b, [0.0, 0.0, 1.0], SH.ball_f32) == (True, 0.0)                   # inside: the entry is the origin
    b2 = SH.ball([0.0, 3.0, 0.0], 1.0)
    assert both(b2, [0.0, 1.0, 0.0], SH.ball_f32) == (True, 2.0)
    assert both(b2, [0.0, -1.0, 0.0], SH.ball_f32) == (False, 0.0)                # behind
    assert both(b2, [1.0, 0.0, 0.0], SH.ball_f32) == (False, 0.0)                 # beside
    bad = b2.copy()
    bad[4] = -1.0
    nan = q.copy()
    nan[9] = np.nan
    flat = q.copy()
    flat[7:10] = flat[4:7]
    for rec in (bad, nan, flat):
        B = SH.body64(x, np.array([[0.0, 1.0, 0.0]]), e0, rec)
        assert B["no"][0] and not B["yes"][0]


def test_analytic_pin_of_the_reference():
    """a ball of angular radius alpha = 0.3 whose centre makes beta = 0.6 with the normal of a floor point of the constant-radiance box (L = 1.5):
    lost = pi L sin^2(alpha) cos(beta) = 0.339661.  At N = 4096 the reference gives 0.336530: deviation 3.1e-3, against the margin of 5 binomial standard
    errors of the blocked share p = 0.04419 (the cap's share of the hemisphere is 1 - cos(alpha) = 0.04466), 5 sqrt(p (1 - p) / N) pi L = 0.0757.
    (Measured on the CPU; nothing of the GPU enters.)"""
    c, want, L = SH.pin_case()
    r = c.ref()
    assert r.caps()[0] == 0
    got = r.scale * r.mid[0].sum(1)[0]
    p = float((np.abs(r.mid[0]).sum(2) > 0).mean())
    margin = 5.0 * math.sqrt(p * (1 - p) / c.N) * math.pi * L
    print("pin: closed form %.6f, reference %s, blocked share %.5f, margin %.4f" % (want, got, p, margin))
    assert abs(p - (1 - math.cos(0.3))) < 5 * math.sqrt(p * (1 - p) / c.N)
    assert (np.abs(got - want) <= margin).all()
    lo, hi = r.scale * r.lo[0].sum(1)[0], r.scale * r.hi[0].sum(1)[0]
    assert (lo <= got).all() and (got <= hi).all()


def test_cover_case_has_at_least_32_texels_on_which_everything_is_blocked():
    """the geometry of the GPU's bit-identity test is chosen here: the texels on which the reference says that every sample with an accepted hit is
    certainly blocked by set {0}; there the restatement's lost IS the estimator's own sum"""
    c = SH.case("box_cover")
    r = c.ref()
    sel = r.all_blocked(0)
    print("box_cover: %d of %d floor texels have every accepted sample certainly blocked" % (sel.sum(), len(sel)))
    assert sel.sum() >= 32
    assert np.array_equal(sel, r.all_blocked(2)) and not r.all_blocked(1).any()
    L, d, t, pid, rad = SH.traced(c)
    full = TC.estimator_f32(c.nrm[L], d, rad.reshape(len(L), c.N, 3), False, "group", c.parts)
    lost, _ = SH.shadow_f32(c)
    assert np.array_equal(lost[0][L][sel].view(np.uint32), full[sel].view(np.uint32))
    assert np.array_equal(lost[0].view(np.uint32), lost[2].view(np.uint32)) and not lost[1][L].any()


# ---- the C-ABI's refusals, without a device --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    from texir_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def shadow_args(**kw):
    a = dict(scene=D, pos=D, nrm=D, shift=D, ids=D, n_ids=64, Nt=100, N=64, mode=0, bodies=D, K=2, sets=D, M=3, out=D, stats=None, ws=D, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ("scene", "pos", "nrm", "shift", "ids", "n_ids", "Nt", "N", "mode", "bodies", "K", "sets", "M", "out", "stats", "ws", "ws_bytes", "stream"))


def refused(L, msg, **kw):
    rc = L.texir_irt_shadow(*shadow_args(**kw))
    got = L.texir_last_error().decode()
    assert rc == INVALID and got.startswith("texir_irt_shadow: " + msg), (kw, rc, got)


def test_cabi_refusals(L):
    refused(L, "K must be in 0..8, got 9", K=9, bodies=None, sets=None, out=None)                # the counts are reported before any null buffer
    refused(L, "K must be in 0..8, got -1", K=-1)
    refused(L, "M must be in 1..8, got 0", M=0, sets=None, out=None)
    refused(L, "M must be in 1..8, got 9", M=9)
    refused(L, "bodies is null", bodies=None)
    refused(L, "sets is null", sets=None)
    for k in ("scene", "pos", "nrm", "shift", "out"):
        refused(L, "null argument", **{k: None})
    refused(L, "mode must be uniform(0) or cosine(1), got 2", mode=2)
    refused(L, "bad sizes N=0", N=0)
    refused(L, "bad sizes N=-3", N=-3)
    refused(L, "bad sizes", n_ids=-1)
    refused(L, "Nt too large", Nt=1 << 31)
    need = 12 * 3 * 8 * 64                                                                         # 12 B x M x parts (N = 64: 8) per listed texel
    assert L.texir_irt_shadow_workspace_bytes(64, 64, 3) == need
    refused(L, "the workspace holds %d bytes, the call needs %d" % (need - 1, need), ws_bytes=need - 1)
    refused(L, "the workspace holds 0 bytes, the call needs %d" % need, ws=None)
    assert L.texir_irt_shadow(*shadow_args(n_ids=0, ws=None, ws_bytes=0)) == 0                      # a non-null empty list is a no-op
    assert L.texir_irt_shadow(*shadow_args(K=0, bodies=None, n_ids=0)) == 0                         # K = 0 needs no records


def test_workspace_bytes(L):
    f = L.texir_irt_shadow_workspace_bytes
    assert f(1, 1, 1) == 12 and f(1, 3, 8) == 96 and f(130, 256, 5) == 12 * 5 * 32 * 130
    for bad in ((0, 64, 1), (-1, 64, 1), (64, 0, 1), (64, 64, 0), (64, 64, 9)):
        assert f(*bad) == 0


# ---- irtlight ----------------------------------------------------------------------------------------------------------------------------------------------------

def _old_add(E, F, colours):
    out = E
    for k in range(F.shape[0]):
        out = out + F[k][..., None] * np.asarray(colours[k], E.dtype).reshape(-1)
    return out


def test_add_and_add_view_without_lost_return_the_bits_they_returned():
    import torch
    from texir_code_amd import irtlight
    rng = np.random.default_rng(5)
    E, F, R = rng.random((6, 7, 3), dtype=F32), rng.random((3, 6, 7), dtype=F32), rng.random((3, 6, 7), dtype=F32)
    alb, G = rng.random((6, 7, 3), dtype=F32), rng.random((3, 6, 7, 3), dtype=F32)
    cols = [(20.0, 18.0, 15.0), 2.0, (0.5, 0.25, 4.0)]
    want = _old_add(E, F, cols)
    assert np.array_equal(irtlight.add(E, F, cols).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(irtlight.add(E, F, cols, lost=None).view(np.uint32), want.view(np.uint32))
    assert torch.equal(irtlight.add(torch.from_numpy(E), torch.from_numpy(F), cols), torch.from_numpy(want))
    pi = np.asarray([irtlight.PI32], F32)
    view = E
    for k in range(3):
        view = view + (alb / pi * F[k][..., None] + R[k][..., None]) * np.asarray(cols[k], F32).reshape(-1)
    assert np.array_equal(irtlight.add_view(E, alb, F, R, cols).view(np.uint32), view.view(np.uint32))
    for k in range(3):
        view = view + (alb / pi * G[k]) * np.asarray(cols[k], F32).reshape(-1)
    assert np.array_equal(irtlight.add_view(E, alb, F, R, cols, G=G, lost=None).view(np.uint32), view.view(np.uint32))


def test_add_with_lost_floors_at_zero_before_the_sum():
    import torch
    from texir_code_amd import irtlight
    rng = np.random.default_rng(6)
    E, F = rng.random((5, 4, 3), dtype=F32), rng.random((2, 5, 4), dtype=F32)
    lost = (rng.random((5, 4, 3), dtype=F32) * F32(1.5)).astype(F32)              # beyond E on part of the image
    cols = [(1.0, 2.0, 3.0), 0.5]
    got = irtlight.add(E, F, cols, lost=lost)
    want = _old_add(np.maximum(E - lost, F32(0)), F, cols)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (lost > E).any()
    assert torch.equal(irtlight.add(torch.from_numpy(E), torch.from_numpy(F), cols, lost=torch.from_numpy(lost)), torch.from_numpy(want))
    assert np.array_equal(irtlight.add(E, F, cols, lost=np.zeros_like(E)).view(np.uint32), _old_add(E, F, cols).view(np.uint32))
    with pytest.raises(ValueError, match="lost"):
        irtlight.add(E, F, cols, lost=lost[:-1])
    # a view: the diffuse term albedo / pi * irr loses albedo / pi * lost, floored with the irradiance at hand
    alb, irr, R = rng.random((5, 4, 3), dtype=F32), rng.random((5, 4, 3), dtype=F32), np.zeros((2, 5, 4), F32)
    pi = np.asarray([irtlight.PI32], F32)
    spec = rng.random((5, 4, 3), dtype=F32)
    rgb = alb / pi * irr + spec
    zero = [0.0, 0.0]
    got = irtlight.add_view(rgb, alb, F, R, zero, lost=lost, irr=irr)
    want = alb / pi * np.maximum(irr - lost, 0) + spec
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(rgb).max() and (got <= rgb).all()
    bare = irtlight.add_view(rgb, alb, F, R, zero, lost=lost)
    assert np.array_equal(bare, np.maximum(rgb - alb / pi * lost, F32(0))) and (bare >= 0).all()


# ---- conf keys, the tool --------------------------------------------------------------------------------------------------------------------------------------------

class _Conf(dict):
    def get(self, k, d=None):
        return dict.get(self, k, d)


def test_conf_keys_parse_and_bad_values_raise(tmp_path):
    from texir_code_amd import models
    from texir_code_amd.conf import ConfigFactory
    from texir_code_amd.tester import lit_model as LM
    assert models.irt_light_shadow_settings(_Conf(), 128) == (False, 128)
    p = tmp_path / "a.conf"
    p.write_text("train {\n    irt_light_shadow = true\n    irt_light_shadow_samples = 32\n}\ntest {\n    light_shadows = true\n    light_shadow_samples = 16\n}\n")
    conf = ConfigFactory.parse_file(str(p))
    assert models.irt_light_shadow_settings(conf, 128) == (True, 32)
    assert LM.light_shadow_settings(conf) == (True, 16)
    assert LM.light_shadow_settings(_Conf()) == (False, 256)
    for bad in ("yes", 1, 0.5, None):
        with pytest.raises(ValueError, match="train.irt_light_shadow must be true or false"):
            models.irt_light_shadow_settings(_Conf({"train.irt_light_shadow": bad}), 64)
        with pytest.raises(ValueError, match="test.light_shadows must be true or false"):
            LM.light_shadow_settings(_Conf({"test.light_shadows": bad}))
    for bad in (0, -4, 2.5, "many", True):
        with pytest.raises(ValueError, match="train.irt_light_shadow_samples"):
            models.irt_light_shadow_settings(_Conf({"train.irt_light_shadow": True, "train.irt_light_shadow_samples": bad}), 64)
        with pytest.raises(ValueError, match="test.light_shadow_samples"):
            LM.light_shadow_settings(_Conf({"test.light_shadow_samples": bad}))
    assert models.light_shadow_sets(1) == [[[0]]]
    assert models.light_shadow_sets(3) == [[[0], [1], [2], [0, 1, 2]]]
    assert models.light_shadow_sets(7) == [[[k] for k in range(7)] + [list(range(7))]]
    assert models.light_shadow_sets(8) == [[[k] for k in range(8)], [list(range(8))]]


def test_light_irt_default_writes_what_it_wrote_and_shadow_subtracts(tmp_path, capsys):
    from texir_code_amd import io_formats as IO, irtlight, tools
    rng = np.random.default_rng(8)
    d = str(tmp_path)
    E = rng.random((8, 8, 3), dtype=F32) + F32(0.5)
    F = rng.random((2, 8, 8), dtype=F32)
    IO.write_hdr(os.path.join(d, "0_irr_texture.hdr"), E)
    for k in range(2):
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d.hdr" % k), np.repeat(F[k][..., None], 3, -1))
    rd = lambda n: np.asarray(IO.read_hdr(os.path.join(d, n)), F32)
    E, F = rd("0_irr_texture.hdr"), np.stack([rd("0_irr_texture_light%d.hdr" % k)[..., 0] for k in range(2)])
    both = ["light-irt", d, "--light", "0", "--colour", "2,2,2", "--light", "1", "--colour", "1,0.5,3"]
    cols = [(2.0, 2.0, 2.0), (1.0, 0.5, 3.0)]
    lit = os.path.join(d, "0_irr_texture_lit.hdr")

    def run(argv):
        if os.path.exists(lit):
            os.remove(lit)
        rc = tools.main(argv)
        return rc, (open(lit, "rb").read() if rc == 0 else None)
    before = sorted(os.listdir(d))
    rc, plain = run(both)
    assert rc == 0 and sorted(os.listdir(d)) == before + ["0_irr_texture_lit.hdr"]
    ref = str(tmp_path / "ref.hdr")
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add(E, F, cols), F32))
    assert plain == open(ref, "rb").read()                                                        # the default: the file it wrote before
    # no shadow files yet: the missing file and the conf key are named
    capsys.readouterr()
    assert run(both + ["--shadow"])[0] == 1
    msg = capsys.readouterr().out
    assert "0_irr_texture_lights_shadow.hdr" in msg and "train.irt_light_shadow" in msg
    assert run(both[:6] + ["--shadow"])[0] == 1
    assert "0_irr_texture_light0_shadow.hdr" in capsys.readouterr().out
    lost = (rng.random((3, 8, 8, 3), dtype=F32) * F32(2)).astype(F32)
    for n, img in (("0_irr_texture_light0_shadow.hdr", lost[0]), ("0_irr_texture_light1_shadow.hdr", lost[1]), ("0_irr_texture_lights_shadow.hdr", lost[2])):
        IO.write_hdr(os.path.join(d, n), img)
    rc, got = run(both + ["--shadow"])
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add(E, F, cols, lost=rd("0_irr_texture_lights_shadow.hdr")), F32))
    assert rc == 0 and got == open(ref, "rb").read() and got != plain
    one = ["light-irt", d, "--light", "1", "--colour", "1,0.5,3", "--shadow"]
    rc, got = run(one)
    IO.write_hdr(ref, np.ascontiguousarray(irtlight.add(E, F[1:], cols[1:], lost=rd("0_irr_texture_light1_shadow.hdr")), F32))
    assert rc == 0 and got == open(ref, "rb").read()
    # a third light in the directory: two named lights are neither one nor all
    IO.write_hdr(os.path.join(d, "0_irr_texture_light2.hdr"), np.repeat(F[0][..., None], 3, -1))
    capsys.readouterr()
    assert run(both + ["--shadow"])[0] == 1
    assert "train.irt_light_shadow" in capsys.readouterr().out
