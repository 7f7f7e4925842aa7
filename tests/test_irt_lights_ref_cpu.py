"""CPU: the float64 reference of the inserted-emitter rule (light_cases) integrates the closed forms, is sharp enough to bind, accepts a float32
restatement of the documented arithmetic and rejects the ways a light pass can go wrong; the helpers of texir_code_amd/irtlight.py; the light-irt command
on hand-written .hdr files; the C-ABI declares and binds the entry point.

  * closed forms at S = 4096, relative bound 2e-3 (five times the worst deviation seen when the rule was written, 3.7e-4; Hammersley error falls about as
    1 / S): a texel under the corner of a 1.2 x 0.9 quad at height 1.5 (pi F_d1-2), a sphere of r = 0.25 straight above at 2 (pi r^2 / h^2) and the same
    sphere off-axis (pi r^2 cos / D^2);
  * the caps of light_cases hold on every case: no overflowing candidate list, uncertain visibility on at most 1 % of the traced samples and in at most
    2 % of the texels;
  * lights_f32 lies inside every interval of every case; each mutant falls out on its case.
"""
import json
import math
import os
import re

import numpy as np
import pytest

import light_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSED_FORM_BOUND = 2e-3
_F32 = {}


def restated(name):
    if name not in _F32:
        _F32[name] = LC.lights_f32(LC.case(name))
    return _F32[name]


# ---- the rule integrates what it should --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.37, 0.81), (0.9, 0.05)])
def test_reference_against_the_closed_forms(shift):
    from texir_code_amd import irtlight
    S, up = 4096, (0.0, 1.0, 0.0)
    # the quad's corner o hangs straight above the texel; a = (1.2, 0, 0), b = (0, 0, 0.9): a x b = (0, -1.08, 0), it shines down
    got = LC.unoccluded_F((0, 0, 0), up, shift, irtlight.quad((0.0, 1.5, 0.0), (1.2, 0.0, 0.0), (0.0, 0.0, 0.9)), S)
    want = LC.corner_form_factor(1.2, 0.9, 1.5)
    assert abs(want - 0.29152870843) < 1e-9
    dev = [abs(got / want - 1)]
    got = LC.unoccluded_F((0, 0, 0), up, shift, irtlight.sphere((0.0, 2.0, 0.0), 0.25), S)
    dev.append(abs(got / (math.pi * 0.25 ** 2 / 4.0) - 1))
    c = np.array([0.8, 1.6, -0.5])
    D2 = float(c @ c)
    got = LC.unoccluded_F((0, 0, 0), up, shift, irtlight.sphere(c, 0.25), S)
    dev.append(abs(got / (math.pi * 0.25 ** 2 * (1.6 / math.sqrt(D2)) / D2) - 1))
    print("closed forms at S = %d, shift %r: relative deviation quad corner %.3e, sphere above %.3e, sphere off-axis %.3e" % ((S, shift) + tuple(dev)))
    assert max(dev) <= CLOSED_FORM_BOUND
    # the quad is one-sided: seen from behind it gives nothing
    assert LC.unoccluded_F((0, 0, 0), up, shift, irtlight.quad((0.0, 1.5, 0.0), (0.0, 0.0, 0.9), (1.2, 0.0, 0.0)), S) == 0.0


def test_sample_points_are_the_device_functions():
    # ham0's two paths, ham1's bit reversal, the wrap and the clamp, pinned on values worked out by hand
    assert LC.ham0_f32(np.array([3]), 16)[0] == np.float32(0.1875) and LC.ham0_f32(np.array([5]), 17)[0] == np.float32(5.0 / 17.0)
    assert LC.ham1_f32(np.array([1, 2, 3, 6]))[:].tolist() == [0.5, 0.25, 0.75, 0.375]
    s = LC.shift_wrap_clamp_f32(np.array([0.75, 0.0, 0.25], np.float32), np.array([0.5, 0.0, 0.75], np.float32))
    assert s[0] == np.float32(0.25) and s[1] == np.float32(1e-6) and s[2] == np.float32(1.0 - 1e-6)      # (0.25 + 0.75 = 1 is not > 1: clamped)


# ---- the reference binds ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LC.ALL)
def test_caps_and_the_float32_restatement(name):
    c = LC.case(name)
    ref = c.ref()
    over, us, ut = ref.caps()
    print("light case %-12s %s" % (name, json.dumps(ref.summary())))
    assert over == 0 and us <= LC.CAP_UNCERTAIN_SAMPLES and ut <= LC.CAP_UNCERTAIN_TEXELS
    F, stats = restated(name)
    fails, worst = LC.check(c, F, stats, LC.SENTINEL)
    print("lights_f32 %-12s worst share of an interval %.3f, stats %s inside %s" % (name, worst, stats.tolist(), ref.counts()))
    assert not fails, fails
    if name == "closed_box":
        assert not F.any() and stats[0] > 0 and stats[1] == 0
    if name == "on_surface":
        assert stats[1] == stats[0] > 0 and (F > 0).any()
    if name == "room_eight":
        assert not F[[1, 3, 4, 5, 6]][:, ref.tex].any() and all((F[k] > 0).any() for k in (0, 2, 7))


@pytest.mark.parametrize("mut", LC.MUTANTS)
def test_mutants_are_rejected(mut):
    c = LC.case(LC.MUTANT_CASES[mut])
    assert not LC.check(c, *restated(c.name))[0]
    F, stats = LC.lights_f32(c, mut)
    fails, _ = LC.check(c, F, stats)
    assert fails, "mutant %s was accepted on %s" % (mut, c.name)
    print("mutant %-18s on %-10s: %s" % (mut, c.name, fails[0]))


def test_the_checker_sees_writes_outside_the_list_and_bad_stats():
    c = LC.case("list65")
    F, stats = restated("list65")
    G = F.copy()
    G[0, np.setdiff1d(np.arange(c.Nt), c.ref().tex)[3]] = 0.0
    assert LC.check(c, G, stats, LC.SENTINEL)[0]
    assert LC.check(c, F, stats + np.array([0, 5]), LC.SENTINEL)[0] or LC.check(c, F, stats - np.array([0, 5]), LC.SENTINEL)[0]


# ---- irtlight.py -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_records_pack_and_refuse():
    from texir_code_amd import irtlight
    q, s = irtlight.quad((1, 2, 3), (1, 0, 0), (0, 0, 2)), irtlight.sphere((4, 5, 6), 0.5)
    assert q.dtype == np.float32 and q.shape == (16,) and np.array_equal(q, LC.quad((1, 2, 3), (1, 0, 0), (0, 0, 2)))
    assert np.array_equal(s, LC.sphere((4, 5, 6), 0.5))
    P = irtlight.pack([q, s])
    assert P.dtype == np.float32 and P.shape == (2, 16) and P.flags["C_CONTIGUOUS"]
    assert irtlight.pack([]).shape == (0, 16)
    assert [LC.record_kind(r) for r in P] == ["quad", "sphere"]
    for bad in (lambda: irtlight.quad((0, 0, 0), (1, 0, 0), (2, 0, 0)), lambda: irtlight.quad((0, 0, float("nan")), (1, 0, 0), (0, 1, 0)),
                lambda: irtlight.quad((0, 0), (1, 0, 0), (0, 1, 0)), lambda: irtlight.sphere((0, 0, 0), 0.0), lambda: irtlight.sphere((0, 0, 0), -1.0),
                lambda: irtlight.sphere((0, 0, 0), float("inf")), lambda: irtlight.pack([q] * 9), lambda: irtlight.pack([q[:15]]),
                lambda: irtlight.pack([np.full(16, 2.0, np.float32)])):
        with pytest.raises(ValueError):
            bad()


def test_load_reads_the_json_form(tmp_path):
    from texir_code_amd import irtlight
    p = tmp_path / "lights.json"
    p.write_text(json.dumps({"lights": [{"kind": "quad", "o": [0, 2.5, 0], "a": [1, 0, 0], "b": [0, 0, 1], "colour": [10, 9, 8]},
                                        {"kind": "sphere", "c": [1, 1, 1], "r": 0.25}]}))
    recs, cols = irtlight.load(str(p))
    assert recs.shape == (2, 16) and recs.dtype == np.float32 and cols.shape == (2, 3) and cols.dtype == np.float32
    assert np.array_equal(recs[0], LC.quad((0, 2.5, 0), (1, 0, 0), (0, 0, 1))) and np.array_equal(recs[1], LC.sphere((1, 1, 1), 0.25))
    assert cols.tolist() == [[10, 9, 8], [1, 1, 1]]
    for doc in ({"lights": [{"kind": "disc", "c": [0, 0, 0], "r": 1}]}, {"lights": [{"kind": "sphere", "c": [0, 0, 0]}]}, {"lamps": []},
                {"lights": [{"kind": "sphere", "c": [0, 0, 0], "r": 1, "colour": [1, 2]}]}, {"lights": [{"kind": "quad", "o": [0, 0, 0], "a": [1, 0, 0], "b": [1, 0, 0]}]}):
        p.write_text(json.dumps(doc))
        with pytest.raises(ValueError):
            irtlight.load(str(p))


def test_add_is_linear_in_numpy_and_torch():
    import torch
    from texir_code_amd import irtlight
    rng = np.random.default_rng(5)
    E, F = rng.random((6, 5, 3), dtype=np.float32), rng.random((2, 6, 5), dtype=np.float32)
    cols = [(2.0, 1.0, 0.5), 3.0]
    got = irtlight.add(E, F, cols)
    want = (E + F[0][..., None] * np.array(cols[0], np.float32)) + F[1][..., None] * np.float32(3.0)
    assert got.dtype == np.float32 and got.shape == E.shape and np.array_equal(got, want)
    gt = irtlight.add(torch.from_numpy(E), torch.from_numpy(F), cols)
    assert torch.is_tensor(gt) and np.array_equal(gt.numpy(), want)
    assert np.array_equal(irtlight.add(E, F[:0], []), E)
    with pytest.raises(ValueError):
        irtlight.add(E, F, cols[:1])
    with pytest.raises(ValueError):
        irtlight.add(E, F[:, :5], cols)


# ---- the command -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_light_irt_command_on_hand_written_files(tmp_path, capsys):
    from texir_code_amd import io_formats as IO, tools
    d = str(tmp_path)
    rng = np.random.default_rng(9)
    E = rng.random((6, 8, 3), dtype=np.float32) + 0.25
    F = [np.repeat(rng.random((6, 8, 1), dtype=np.float32), 3, 2) for _ in range(2)]
    other = rng.random((6, 8, 3), dtype=np.float32) * 4
    IO.write_hdr(os.path.join(d, "0_irr_texture.hdr"), E)
    IO.write_hdr(os.path.join(d, "0_irr_texture_relit.hdr"), other)
    for k in range(2):
        IO.write_hdr(os.path.join(d, "0_irr_texture_light%d.hdr" % k), F[k])
    rd = lambda f: IO.read_hdr(os.path.join(d, f)).astype(np.float64)
    E_, O_, F_ = rd("0_irr_texture.hdr"), rd("0_irr_texture_relit.hdr"), [rd("0_irr_texture_light%d.hdr" % k) for k in range(2)]
    lit = os.path.join(d, "0_irr_texture_lit.hdr")
    # an RGBE pixel keeps 8 bits below its largest channel's power of two: the written sum is off by at most 2^-7 of that channel (and float32 roundings)
    close = lambda got, want: (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    assert tools.main(["light-irt", d, "--light", "1", "--colour", "2,1,0.5"]) == 0
    assert close(rd("0_irr_texture_lit.hdr"), E_ + F_[1] * np.array([2.0, 1.0, 0.5]))
    assert tools.main(["light-irt", d, "--light", "1", "--colour", "2,1,0.5"]) == 1 and "not overwritten" in capsys.readouterr().out
    os.remove(lit)
    assert tools.main(["light-irt", d, "--light=0", "--colour=4,4,4", "--light", "1", "--colour", "0,1,3"]) == 0                   # two lights
    assert close(rd("0_irr_texture_lit.hdr"), E_ + 4.0 * F_[0] + F_[1] * np.array([0.0, 1.0, 3.0]))
    os.remove(lit)
    assert tools.main(["light-irt", d, "--light", "0", "--colour", "1,1,1", "--base", os.path.join(d, "0_irr_texture_relit.hdr")]) == 0
    assert close(rd("0_irr_texture_lit.hdr"), O_ + F_[0])
    os.remove(lit)
    capsys.readouterr()
    assert tools.main(["light-irt", d, "--light", "2", "--colour", "1,1,1"]) == 1
    assert "0_irr_texture_light2.hdr" in capsys.readouterr().out and not os.path.exists(lit)
    assert tools.main(["light-irt", d, "--light", "0", "--colour", "1,1,1", "--base", os.path.join(d, "nothing.hdr")]) == 1
    assert "nothing.hdr" in capsys.readouterr().out
    for bad in (["light-irt", d], ["light-irt", d, "--light", "0"], ["light-irt", d, "--light", "0", "--colour", "1,1"], ["light-irt", d, "--colour", "1,1,1"],
                ["light-irt", d, "--light", "0", "--colour", "1,1,1", "--replace"]):
        assert tools.main(bad) == 2
    assert not os.path.exists(lit)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_the_loader_binds_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    m = re.search(r"TEXIR_API int texir_irt_lights\(([^;]*)\);", hdr)
    assert m, "texir_irt_lights is not declared"
    n_args = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
    assert n_args == 14
    for word in ("FLOAT32 OPERATION SEQUENCE", "ROUNDING BOUND", "shift_wrap_clamp", "t_max"):
        assert word in hdr[hdr.index("inserted emitters"):m.start()]
    from texir_code_amd import _lib
    assert len(_lib.signatures()["texir_irt_lights"]) == n_args
    mk = open(os.path.join(ROOT, "texir_code_amd", "csrc", "Makefile")).read()
    assert mk.count("irtlight.hip") == 2
    from texir_code_amd import scene
    assert callable(scene.Scene.irt_lights)
