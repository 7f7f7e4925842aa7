"""irt_shadow_kernel (csrc/irtshadow.hip) and irt_combine_kernel (csrc/kernels.hip) behind texir_irt_shadow, Scene.irt_shadow, irtlight.add(lost=), the IrT
stage's train.irt_light_shadow, `light-irt --shadow` and the evaluation model's test.light_shadows, on the golden box (12 triangles) and room (20 k).

  1. intervals   every case of irt_shadow_cases inside its float64 reference, stats inside its counts, unlisted texels untouched: lists of 1, 63, 65, 130
                 and 165 texels, N in 1, 3, 64, 256 (1, 8 and 32 parts, the natural order), K in 0, 1, 2, 3, 8, M in 1, 2, 3, 5, 8, both sample modes;
                 passes no lane, one lane and every lane of which meets a body; a body behind the scene's hit; a sheet edge-on to grazing rays; a quad met
                 from its back; texels inside a ball; a body met only by rays that leave an open scene; an invalid and a NaN record among valid ones; a
                 zero mask; a mask with bits at or above K; overlapping bodies with the sets {0}, {1}, {0, 1};
  2. bits        where the reference says every accepted sample is blocked, lost IS irt_generate in its 64-texel form (a cover above the floor, a ball
                 around everything; 1, 2, 8 and 32 parts); bodies no ray meets give +0 and stats == 0; a far body in the set changes no bit;
  3. purity      permuted, duplicated and cut lists, a side stream, several slices: identical bits; a recorded graph replayed after the records were
                 overwritten on the device returns the bits of a fresh call with the new records;
  4. errors      every refused argument raises;
  5. end to end  the stage's files, `light-irt --shadow`, the evaluation model.
The cosine ESTIMATOR (mode | 4 inside the library) has no case: the entry point takes texir_irt_generate's public `mode`, which cannot name it.
"""
import json
import os

import numpy as np
import pytest
import torch

import irt_shadow_cases as SH
import trace_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL = SH.SENTINEL
GROUP = "irt_group_kernel<false, 4, 6>"
_SC, _DEV = {}, {}


def scene_of(tx, geo):
    if geo.name not in _SC:
        _SC[geo.name] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    return _SC[geo.name]


def dev_inputs(c):
    key = (c.geo.name, c.Nt)
    if key not in _DEV:
        _DEV[key] = tuple(torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.shift))
    return _DEV[key]


def masks_of(c):
    """the sets as the call takes them, raw: bits at or above K included"""
    return torch.from_numpy(np.array(c.sets, np.uint32).view(np.int32)).cuda()


def shadow(tx, c, ids=None, bodies=None, **kw):
    pos, nrm, shift = dev_inputs(c)
    out = torch.full((c.M, c.Nt, 3), SENTINEL, device="cuda")
    ids = torch.from_numpy(c.ids).cuda() if ids is None else ids
    bodies = torch.from_numpy(c.bodies).cuda() if bodies is None else bodies
    got, st = scene_of(tx, c.geo).irt_shadow(pos, nrm, shift, c.N, bodies, sets=masks_of(c), mode=c.mode, texel_ids=ids, out=out, stats=True, **kw)
    assert got is out
    return out.cpu().numpy(), st.cpu().numpy()


def generate(tx, c):
    pos, nrm, shift = dev_inputs(c)
    sc = scene_of(tx, c.geo)
    assert sc.irt_kernel_name(len(c.ids), c.N) == GROUP
    out = torch.full((c.Nt, 3), SENTINEL, device="cuda")
    return sc.irt_generate(pos, nrm, shift, c.N, c.mode, texel_ids=torch.from_numpy(c.ids).cuda(), out=out).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. intervals ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SH.GPU_CASES)
def test_every_case_inside_its_float64_reference(tx, name):
    c = SH.case(name)
    lost, st = shadow(tx, c)
    worst = SH.check(c, lost, st, SENTINEL, "gpu")
    print("irt_shadow %s: worst share of the interval %.4f, stats %s, reference counts %s" % (name, worst, st.tolist(), c.ref().counts()))
    assert worst <= 1.0


def test_the_cases_cover_what_they_claim():
    """read off the reference alone: lists, N, parts, K, M; passes met by no lane, one lane, every lane; bodies behind the hit; texels inside a ball"""
    cs = [SH.case(n) for n in SH.GPU_CASES]
    assert {1, 63, 65, 130} <= {len(c.ids) for c in cs} and {1, 3, 64, 256} <= {c.N for c in cs} and {1, 8, 32} <= {c.parts for c in cs}
    assert {0, 1, 3, 8} <= {c.K for c in cs} and {1, 2, 5, 8} <= {c.M for c in cs} and {"uniform", "cosine"} <= {c.mode for c in cs}
    r = SH.case("box_eight").ref()
    assert (SH.case("box_below").ref().meet_maybe.sum() == 0) and (SH.case("box_inside").ref().meet_yes.all())
    # the tiny ball alone: 65 texels are two waves, 256 passes each; it is met by a handful of samples, so nearly every pass meets it in no lane and the
    # few others in one lane or little more
    tiny = SH.Case("tiny", r.case.geo, r.case.pos, r.case.nrm, r.case.shift, r.case.ids, r.case.N, r.case.mode, r.case.bodies[6:7], [1]).ref()
    assert 1 <= tiny.meet_yes.sum() and tiny.meet_maybe.sum() <= 8 < 2 * r.case.N
    three = SH.case("box_three").ref()
    assert three.meet_yes.sum() > three.blk_maybe.sum() > 0, "met but not blocked: the body behind the wall"
    assert not np.abs(three.mid[2]).any() and np.abs(three.mid[0]).any()
    assert not np.abs(SH.case("box_open_top").ref().mid[0]).any() and SH.case("box_open_top").ref().meet_yes.sum() > 0


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------------------------------------

def test_where_everything_is_blocked_lost_is_irt_generate_bit_for_bit(tx, monkeypatch):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    c = SH.case("box_cover")
    r = c.ref()
    sel = r.all_blocked(0)
    assert sel.sum() >= 32
    lost, st = shadow(tx, c)
    want = generate(tx, c)
    rows = r.tex[sel]
    assert np.array_equal(bits(lost[0][rows]), bits(want[rows])), "%d of %d texels differ" % ((bits(lost[0][rows]) != bits(want[rows])).any(1).sum(), len(rows))
    assert (want[rows] > 0).any()
    # the far body alone: met by a few rays, never in front of a wall: exactly +0; in the set with the cover: no bit changes
    assert not bits(lost[1][r.tex]).any() and np.array_equal(bits(lost[0]), bits(lost[2]))
    print("box_cover: %d texels equal irt_generate bit for bit; stats %s" % (len(rows), st.tolist()))


@pytest.mark.parametrize("name,switch,value,parts", [("box_inside", None, None, 1), ("box_inside256", None, None, 32), ("box_inside256", "TEXIR_IRT_MIN_PART_CELLS", "128", 2),
                                                      ("box_inside256", "TEXIR_IRT_LOG2PARTS", "3", 8), ("box_one", None, None, 1)])
def test_a_ball_around_everything_returns_irt_generate(tx, monkeypatch, name, switch, value, parts):
    from texir_code_amd import _lib
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    if switch:
        monkeypatch.setenv(switch, value)
    c = SH.case(name)
    assert int(_lib.lib().texir_irt_shadow_workspace_bytes(1, c.N, c.M)) == 12 * c.M * parts
    lost, st = shadow(tx, c)
    want = generate(tx, c)
    sel = c.ref().all_blocked(0)                                              # (all but a texel with a sample in doubt: one of 65 at N = 256)
    rows = c.ref().tex[sel]
    assert sel.sum() >= len(sel) - 1
    assert np.array_equal(bits(lost[0][rows]), bits(want[rows])) and (want[rows] > 0).any()
    lo, hi = c.ref().counts()[2:]
    assert st[0] == len(c.ids) * c.N and lo <= st[1] <= hi


def test_bodies_no_ray_meets_give_plus_zero_and_no_ray_is_traced(tx):
    c = SH.case("box_below")
    lost, st = shadow(tx, c)
    assert not bits(lost[:, c.ref().tex]).any() and st.tolist() == [0, 0]
    assert (lost[:, np.setdiff1d(np.arange(c.Nt), c.ref().tex)] == SENTINEL).all()
    c0 = SH.case("box_nobody")
    lost, st = shadow(tx, c0)
    assert not bits(lost[:, c0.ref().tex]).any() and st.tolist() == [0, 0]


# ---- 3. purity ---------------------------------------------------------------------------------------------------------------------------------------------

def test_result_is_a_pure_function_of_the_inputs(tx):
    from texir_code_amd import _lib
    c = SH.case("box_three")
    base, st = shadow(tx, c)
    ids = torch.from_numpy(c.ids).cuda()
    n = len(c.ids)
    again, st2 = shadow(tx, c)
    assert np.array_equal(bits(base), bits(again)) and st.tolist() == st2.tolist(), "second run"
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    assert np.array_equal(bits(base), bits(shadow(tx, c, ids[perm])[0])), "permuted list"
    dup, st_dup = shadow(tx, c, torch.cat([ids, ids[:40]]))
    assert np.array_equal(bits(base), bits(dup)), "duplicated entries"
    cut = torch.full((c.M, c.Nt, 3), SENTINEL, device="cuda")
    pos, nrm, shift = dev_inputs(c)
    for part in (ids[:1], ids[1:70], ids[70:]):
        scene_of(tx, c.geo).irt_shadow(pos, nrm, shift, c.N, torch.from_numpy(c.bodies).cuda(), sets=masks_of(c), mode=c.mode, texel_ids=part, out=cut)
    assert np.array_equal(bits(base), bits(cut.cpu().numpy())), "cut lists"
    per_texel = int(_lib.lib().texir_irt_shadow_workspace_bytes(1, c.N, c.M))
    assert per_texel == 12 * c.M * c.parts
    sliced, st_sl = shadow(tx, c, max_workspace_bytes=64 * per_texel)
    assert np.array_equal(bits(base), bits(sliced)) and st_sl.tolist() == st.tolist(), "three slices (64 + 64 + 2 texels)"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, _ = shadow(tx, c)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(base), bits(on_side)), "side stream"
    # the friendly form of the sets: lists of body indices
    out = scene_of(tx, c.geo).irt_shadow(pos, nrm, shift, c.N, c.bodies, sets=[[0], [1], [2], [0, 1, 2], [0, 1]], mode=c.mode, texel_ids=ids)
    assert np.array_equal(bits(base[:, c.ref().tex]), bits(out.cpu().numpy()[:, c.ref().tex])), "sets as index lists"
    dflt = scene_of(tx, c.geo).irt_shadow(pos, nrm, shift, c.N, c.bodies, texel_ids=ids)
    assert tuple(dflt.shape) == (3, c.Nt, 3) and np.array_equal(bits(dflt.cpu().numpy()[:, c.ref().tex]), bits(base[:3, c.ref().tex])), "default: one set per body"


def test_a_replayed_graph_sees_the_records_the_device_holds_then(tx):
    from texir_code_amd import _lib
    c = SH.case("box_three")
    L = _lib.lib()
    sc = scene_of(tx, c.geo)
    pos, nrm, shift = dev_inputs(c)
    ids = torch.from_numpy(c.ids).cuda()
    n, Nt, M, K, guard = len(c.ids), c.Nt, c.M, c.K, 64
    bodies = torch.from_numpy(c.bodies).cuda()
    masks = masks_of(c)
    out = torch.full((M * Nt * 3 + guard,), SENTINEL, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    need = int(L.texir_irt_shadow_workspace_bytes(n, c.N, M))
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    base, st0 = shadow(tx, c)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                               # the single call on one stream: no parallel branches
            _lib.check(L.texir_irt_shadow(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n, Nt, c.N, 0, _lib.ptr(bodies), K, _lib.ptr(masks), M,
                                          _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws), need, _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)

    def replay(want, want_st, what):
        out.fill_(SENTINEL)
        stats.zero_()
        ws[:need].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(want), bits(out[:M * Nt * 3].reshape(M, Nt, 3).cpu().numpy())), what
        assert stats.cpu().tolist() == want_st.tolist(), what
        assert (out[M * Nt * 3:] == SENTINEL).all() and (ws[need:] == 0xA5).all(), "guard words"
    replay(base, st0, "graph replay")
    replay(base, st0, "second graph replay")
    moved = c.bodies.copy()
    moved[0, 1:4] += np.array([1.5, -1.0, 0.75], np.float32)                 # the panel, lower and elsewhere
    moved[1, 4] = 0.9                                                         # the ball, larger
    moved[2] = SH.ball([4.0, 2.0, 1.0], 0.4)                                  # the outside ball comes inside
    bodies.copy_(torch.from_numpy(moved))
    fresh, st1 = shadow(tx, c, bodies=torch.from_numpy(moved).cuda())
    assert not np.array_equal(bits(fresh), bits(base)) and np.abs(fresh[2][c.ref().tex]).any()
    replay(fresh, st1, "graph replay after the records were overwritten on the device")


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise(tx, monkeypatch):
    from texir_code_amd import _lib
    c = SH.case("box_three")
    sc = scene_of(tx, c.geo)
    pos, nrm, shift = dev_inputs(c)
    ids = torch.from_numpy(c.ids).cuda()[:65]
    with pytest.raises(_lib.TexirError, match="K must be in 0..8, got 9"):
        sc.irt_shadow(pos, nrm, shift, 64, torch.zeros((9, 16)), sets=[[0]], texel_ids=ids)
    with pytest.raises(_lib.TexirError, match="M must be in 1..8, got 9"):
        sc.irt_shadow(pos, nrm, shift, 64, c.bodies, sets=[[0]] * 9, texel_ids=ids)
    with pytest.raises(_lib.TexirError, match="M must be in 1..8, got 0"):
        sc.irt_shadow(pos, nrm, shift, 64, c.bodies[:0], texel_ids=ids)       # the default sets of no body: none
    for bad_n in (0, -64):
        with pytest.raises(_lib.TexirError, match="bad sizes"):
            sc.irt_shadow(pos, nrm, shift, bad_n, c.bodies, texel_ids=ids)
    with pytest.raises(ValueError, match="bodies must be"):
        sc.irt_shadow(pos, nrm, shift, 64, c.bodies[:, :12], texel_ids=ids)
    with pytest.raises(ValueError, match="indices are 0..31"):
        sc.irt_shadow(pos, nrm, shift, 64, c.bodies, sets=[[32]], texel_ids=ids)
    with pytest.raises(ValueError, match="out must be"):
        sc.irt_shadow(pos, nrm, shift, 64, c.bodies, texel_ids=ids, out=torch.zeros((2, c.Nt, 3), device="cuda"))
    out = torch.full((3, c.Nt, 3), SENTINEL, device="cuda")
    assert sc.irt_shadow(pos, nrm, shift, 64, c.bodies, texel_ids=ids[:0], out=out) is out      # an empty list never reaches the library
    L = _lib.lib()
    need = int(L.texir_irt_shadow_workspace_bytes(65, 64, 3))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    bodies, masks = torch.from_numpy(c.bodies).cuda(), masks_of(c)[:3].contiguous()
    call = lambda n_ids, w, nbytes, s=sc: L.texir_irt_shadow(s.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, c.Nt, 64, 0, _lib.ptr(bodies), 3,
                                                           _lib.ptr(masks), 3, _lib.ptr(out), None, _lib.ptr(w), nbytes, _lib.stream_ptr())
    with pytest.raises(_lib.TexirError, match="workspace"):
        _lib.check(call(65, ws, need - 1))
    with pytest.raises(_lib.TexirError, match="workspace"):
        _lib.check(call(65, None, need))
    _lib.check(call(0, None, 0))                                              # a non-null empty list is a no-op, whatever the workspace
    monkeypatch.setenv("TEXIR_BVH_WIDTH", "2")
    binary = tx.Scene(c.geo.verts, c.geo.tris, c.geo.tri_uvs, c.geo.hdr)
    with pytest.raises(_lib.TexirError, match="4-wide tree"):
        _lib.check(call(65, ws, need, binary))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------------------------

def test_stage_writes_the_shadow_files_and_light_irt_subtracts_them(tmp_path, capsys):
    from texir_code_amd import datasets as D, io_formats as IO, irtlight, tools
    from texir_code_amd.trainer import exp_runner as ER

    def stage(tag, extra):
        root = str(tmp_path / tag)
        D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
        conf = str(tmp_path / (tag + ".conf"))
        D.write_conf(conf, root, cube_res=16, spp=(64, 16), model="irt")
        txt = open(conf).read()
        assert "batch_size = 1" in txt
        with open(conf, "w") as f:
            f.write(txt.replace("batch_size = 1", "batch_size = 1\n    " + "\n    ".join(extra), 1))
        d = os.path.join(root, "vrproc", "hdr_texture")
        before = set(os.listdir(d))
        ER.main(["--conf", conf, "--trainstage", "IrrT", "--gpu", "0"])
        return d, {f: open(os.path.join(d, f), "rb").read() for f in sorted(set(os.listdir(d)) - before)}

    probe = str(tmp_path / "probe")
    D.write_synthetic_dataset(probe, T=2000, texel_res=64, tex_res=64, n_side=2)
    verts = np.array([[float(v) for v in l.split()[1:4]] for l in open(os.path.join(probe, "vrproc", "hdr_texture", "out1.obj")) if l.startswith("v ")])
    lo, hi = verts.min(0), verts.max(0)
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.3 * ext[0], 0, 0], [0, 0, 0.3 * ext[2]]
    spec = {"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                       {"kind": "sphere", "c": [ctr[0], lo[1] + 0.5 * ext[1], ctr[2]], "r": 0.12 * float(ext.min())}]}
    js = str(tmp_path / "lights.json")
    with open(js, "w") as f:
        json.dump(spec, f)
    lights = ['irt_lights = "%s"' % js, "irt_light_samples = 16"]
    d0, plain = stage("plain", lights)
    d1, off = stage("off", lights + ["irt_light_shadow = false"])
    d2, on = stage("on", lights + ["irt_light_shadow = true"])
    assert not [f for f in plain if "shadow" in f]
    assert sorted(off) == sorted(plain) and all(off[f] == plain[f] for f in plain), "the default: every file unchanged"
    assert sorted(set(on) - set(plain)) == ["0_irr_texture_light0_shadow.hdr", "0_irr_texture_light1_shadow.hdr", "0_irr_texture_lights_shadow.hdr"]
    assert all(on[f] == plain[f] for f in plain), "0_irr_texture.hdr and the lights' files are byte-identical with and without the key"
    rd = lambda name: IO.read_hdr(os.path.join(d2, name)).astype(np.float32)
    E = rd("0_irr_texture.hdr")
    F = np.stack([rd("0_irr_texture_light%d.hdr" % k)[..., 0] for k in (0, 1)])
    S = [rd("0_irr_texture_light%d_shadow.hdr" % k) for k in (0, 1)]
    U_ = rd("0_irr_texture_lights_shadow.hdr")
    rgbe = lambda x: 2.0 ** -7 * x.max(-1)[..., None] + 1e-6                  # an RGBE pixel keeps 8 bits below its largest channel's power of two
    for k in (0, 1):
        assert S[k].shape == E.shape and S[k].max() > 0
        # the same samples at the same count: a part of the irradiance, never more; the union is at least each lamp's and at most their sum
        assert (S[k] <= E + rgbe(E) + rgbe(S[k])).all() and (U_ >= S[k] - rgbe(U_) - rgbe(S[k])).all()
        with capsys.disabled():
            print("stage: light %d: its body takes up to %.1f %% of a texel's irradiance, from %.1f %% of the atlas" %
                  (k, 100 * float((S[k].sum(-1) / np.maximum(E.sum(-1), 1e-9)).max()), 100.0 * (S[k].sum(-1) > 0).mean()))
    assert (U_ <= S[0] + S[1] + rgbe(U_) + rgbe(S[0]) + rgbe(S[1])).all() and (U_ <= E + rgbe(E) + rgbe(U_)).all()
    cols = [(20.0, 18.0, 15.0), (5.0, 5.0, 9.0)]
    argv = ["light-irt", d2, "--light", "0", "--colour", "20,18,15", "--light", "1", "--colour", "5,5,9"]
    assert tools.main(argv) == 0
    direct = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    os.remove(os.path.join(d2, "0_irr_texture_lit.hdr"))
    assert tools.main(argv + ["--shadow"]) == 0
    got = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    want = irtlight.add(E, F, cols, lost=U_).astype(np.float64)
    assert (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    assert (got <= direct + 2.0 ** -6 * direct.max(-1)[..., None]).all() and got.sum() < direct.sum()
    os.remove(os.path.join(d2, "0_irr_texture_lit.hdr"))
    assert tools.main(argv[:6] + ["--shadow"]) == 0
    got = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    want = irtlight.add(E, F[:1], cols[:1], lost=S[0]).astype(np.float64)
    assert (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    capsys.readouterr()
    assert tools.main(["light-irt", d0, "--light", "0", "--colour", "1,1,1", "--shadow"]) == 1          # no shadow files there
    assert "train.irt_light_shadow" in capsys.readouterr().out


def test_evaluation_model_with_light_shadows_is_nowhere_brighter_in_its_diffuse_term(tx, tmp_path):
    from texir_code_amd import cameras, gbuffer as GB, irtlight
    from texir_code_amd.tester import lit_model as LM, test_model as TM
    from texir_code_amd.texture import texture as tex_fetch
    geo, _ = TC.golden_geo("room")
    full = scene_of(tx, geo)
    lo, hi = geo.verts.min(0).astype(np.float64), geo.verts.max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.3 * ext[0], 0, 0], [0, 0, 0.3 * ext[2]]
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                                         {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.1 * float(ext.min())}]}))
    R = 64
    g = torch.Generator().manual_seed(12)
    par = lambda t: torch.nn.Parameter(t.cuda(), requires_grad=False)
    m = LM.MaterialModel.__new__(LM.MaterialModel)
    torch.nn.Module.__init__(m)
    m.scene, m.device = full, full.device
    m.sample_l, m.sample_type, m.relighting, m.cube_res = [16, 16], ["uniform", "importance"], False, 8
    m.materials_a = par(0.1 + 0.7 * torch.rand(R, R, 3, generator=g))
    m.materials_r = par(0.2 + 0.5 * torch.rand(R, R, 1, generator=g))
    m.irrt = par(0.5 + torch.rand(R, R, 3, generator=g))
    m.texture_seg = par(torch.zeros(R, R, 1))
    m.max_mip_level = TM.get_mip_level(R)
    m._gb_cache = {}
    m.test_lights, m.light_samples = LM.load_test_lights(str(js), m.device), 32
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = ctr
    mvp, cam = cameras.cube_mvps(E)
    torch.manual_seed(5)
    absent = m(mvp, "v", cam, False)                                       # the attributes of the shadow absent: the model as it was
    state = torch.get_rng_state()
    m.light_shadows, m.light_shadow_samples, m.shadow_tex = False, 64, None
    torch.manual_seed(5)
    off = m(mvp, "v", cam, False)
    assert torch.equal(torch.get_rng_state(), state)
    assert sorted(off) == sorted(absent) and all(torch.equal(off[k], absent[k]) for k in off), "the default: the same outputs"
    m.light_shadows = True
    torch.manual_seed(5)
    before = torch.get_rng_state()
    tex = m.build_shadow_texture()
    assert torch.equal(torch.get_rng_state(), before), "the texel shifts drew from the CPU generator"
    assert tuple(tex.shape) == (R, R, 3) and tex.is_cuda and (tex > 0).any() and (tex >= 0).all() and torch.isfinite(tex).all()
    lit = m(mvp, "v", cam, False)
    assert torch.equal(torch.get_rng_state(), state) and getattr(m, "_shadow_irr", None) is None
    # the texture restated from the pieces: the union of both bodies on irt.hdr's grid, the bounce texture's texel G-buffer and private generator
    records, colours = m.test_lights
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(full, R, R, normal="geometric", offset=1e-2, want_ids=True)
    ids = torch.nonzero((prim >= 0).reshape(-1))[:, 0].to(torch.int32)
    shift = torch.rand(R * R, 2, generator=torch.Generator().manual_seed(LM.BOUNCE_SEED)).cuda()
    lost = full.irt_shadow(pos.reshape(-1, 3), nrm.reshape(-1, 3), shift, 64, records, sets=[[0, 1]], texel_ids=ids)
    assert torch.equal(tex, lost[0].reshape(R, R, 3))
    # the view: the diffuse term albedo / pi32 * irr loses albedo / pi32 * (irr - max(irr - lost, 0)): nowhere brighter, somewhere darker
    gb = m._gbuffer(mvp, "v")
    fetch = tex_fetch(tex, gb["uv"], gb["uv_da"], "linear-mipmap-linear", m.max_mip_level)
    irr = tex_fetch(m.irrt, gb["uv"], gb["uv_da"], "linear-mipmap-linear", m.max_mip_level)
    pi = torch.tensor([irtlight.PI32], device="cuda")
    drop = (lit["albedo"] / pi * (irr - (irr - fetch).clamp(min=0))).double()
    want = off["rgb"].double() - drop
    ulp = torch.from_numpy(np.spacing(np.abs(off["rgb"].double().cpu().numpy()).astype(np.float32))).cuda().double()
    assert (fetch > 0).any() and (drop >= 0).all()
    assert ((lit["rgb"].double() - want).abs() <= 4 * ulp).all()
    assert (lit["rgb"] <= off["rgb"]).all() and (lit["rgb"] < off["rgb"]).any()
    for k in ("albedo", "normal", "position", "roughness", "empty_mask"):
        assert torch.equal(lit[k], off[k])
