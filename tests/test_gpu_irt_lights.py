"""irt_lights_kernel (csrc/irtlight.hip) behind texir_irt_lights, Scene.irt_lights, the IrT stage's train.irt_lights and the light-irt command.

  1. intervals    every listed texel of every case of light_cases (S in 1, 2, 16, 17, 64; lists of 1 / 63 / 64 / 65 / 200 texels, a NULL list, K = 8 mixed
                  records, the closed box, the light lying on a surface) inside the float64 reference's interval, stats inside its counts, unlisted texels
                  untouched; one case again on the binary tree;
  2. restatement  against lights_f32: whether the bits agree is reported; binding is agreement within the header's rounding bound on every texel whose
                  samples are all certain;
  3. the route    room_quad and room_sphere against rays built in torch + trace_shade(return_hits=True) + a torch reduction in the rule's order,
                  relative L2 <= 1e-3 (the project's parity bound);
  4. purity       shuffled list, second run, side stream, a captured graph replayed twice: identical bits; the replay after the device records were
                  overwritten with a moved light equals a direct call with the moved light; guard words behind F intact;
  5. errors       every refused argument raises TexirError; K = 0 and an empty list write nothing;
  6. linearity    irtlight.add with two colours equals the sum of two one-light calls bit for bit;
  7. stage        train.irt_lights = <json> writes 0_irr_texture_light<k>.hdr; with `none` the directory is that of a run without the key, byte for byte;
                  light-irt round-trips from those files.
"""
import json
import os

import numpy as np
import pytest
import torch

import light_cases as LC

pytestmark = pytest.mark.gpu

_SC = {}


def scene_of(tx, geo, tag=""):
    key = (geo.name, tag)
    if key not in _SC:
        _SC[key] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    return _SC[key]


def run(tx, c, lights=None, ids="case", tag="", **kw):
    """-> (F [K,Nt] numpy, stats [2] numpy) with the sentinel in every texel the call does not write"""
    sc = scene_of(tx, c.geo, tag)
    lights = c.lights if lights is None else lights
    out = torch.full((lights.shape[0], c.Nt), LC.SENTINEL, device="cuda")
    ids = c.ids if isinstance(ids, str) else ids
    F, st = sc.irt_lights(torch.from_numpy(c.pos).cuda(), torch.from_numpy(c.nrm).cuda(), torch.from_numpy(c.shift).cuda(), torch.from_numpy(lights), c.S,
                          texel_ids=None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda(), t_max=c.t_max, out=out, stats=True, **kw)
    assert F is out
    return F.cpu().numpy(), st.cpu().numpy()


# ---- 1. intervals ------------------------------------------------------------------------------------------------------------------------------------------

def inside(tx, name, tag=""):
    c = LC.case(name)
    F, st = run(tx, c, tag=tag)
    fails, worst = LC.check(c, F, st, LC.SENTINEL)
    print("irt_lights %-12s%s S=%-3d K=%d: worst share of an interval %.3f; stats %s inside %s" % (name, tag, c.S, c.K, worst, st.tolist(), c.ref().counts()))
    assert not fails, fails
    return c, F, st


@pytest.mark.parametrize("name", LC.ALL)
def test_every_listed_texel_inside_the_float64_reference(tx, name):
    c, F, st = inside(tx, name)
    if name == "closed_box":
        assert not F.any() and st[0] > 0 and st[1] == 0
    if name == "on_surface":
        assert st[1] == st[0] > 0 and (F > 0).any()
    if name == "room_eight":
        assert not F[[1, 3, 4, 5, 6]][:, c.ref().tex].any() and all((F[k][c.ref().tex] > 0).any() for k in (0, 2, 7))


def test_the_binary_tree_gives_values_inside_the_reference_too(tx, monkeypatch):
    c = LC.case("list200")
    wide, _ = run(tx, c)                                                   # (the shared 4-wide scene is built before the switch is set)
    monkeypatch.setenv("TEXIR_BVH_WIDTH", "2")
    binary = tx.Scene(c.geo.verts, c.geo.tris, c.geo.tri_uvs, c.geo.hdr)     # kept out of the shared cache
    _SC[(c.geo.name, " (binary tree)")] = binary
    try:
        _, F, _ = inside(tx, "list200", tag=" (binary tree)")
    finally:
        del _SC[(c.geo.name, " (binary tree)")]
    print("irt_lights list200: binary tree and 4-wide tree agree bit for bit: %s" % np.array_equal(F, wide))


# ---- 2. the float32 restatement ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["list63", "list65", "null200", "on_surface", "closed_box"])
def test_agrees_with_the_float32_restatement(tx, name):
    c = LC.case(name)
    F, st = run(tx, c)
    R, rst = LC.lights_f32(c)
    tex = c.ref().tex
    same = np.array_equal(F.view(np.uint32), R.view(np.uint32))
    diff = np.abs(F[:, tex].astype(np.float64) - R[:, tex].astype(np.float64))
    sure = LC.all_certain(c)
    bound = LC.rounding_bound(c)
    with np.errstate(all="ignore"):
        share = np.where(sure & (bound > 0), diff / bound, 0.0)
    print("irt_lights %-10s against lights_f32: bits %s; %d of %d values differ, worst share of the rounding bound %.3f; stats %s / %s"
          % (name, "agree" if same else "differ", int((diff > 0).sum()), diff.size, float(share.max()) if share.size else 0.0, st.tolist(), rst.tolist()))
    assert (diff[sure] <= bound[sure]).all()
    assert (F[:, np.setdiff1d(np.arange(c.Nt), tex)] == LC.SENTINEL).all()


# ---- 3. the route without the kernel -------------------------------------------------------------------------------------------------------------------------------

def torch_route(sc, c):
    """the same rule from rays built in torch (float32, one rounded operation per torch op), Scene.trace_shade and a reduction in ascending i"""
    L = torch.from_numpy(np.unique(c.listed())).cuda()
    x, n = torch.from_numpy(c.pos).cuda()[L], torch.from_numpy(c.nrm).cuda()[L]
    s0, s1 = (torch.from_numpy(a).cuda() for a in LC.sample_points(c.shift[L.cpu().numpy()], c.S))
    out = torch.zeros((c.K, c.Nt), device="cuda")
    for k in range(c.K):
        rec = torch.from_numpy(c.lights[k]).cuda()
        kind = LC.record_kind(c.lights[k])
        o, a, b = rec[1:4], rec[4:7], rec[7:10]
        if kind == "quad":
            y = (o + s0[..., None] * a) + s1[..., None] * b
            m = torch.linalg.cross(a, b).expand_as(y)
            w = 1.0
        else:
            z = 1 - 2 * s0
            q = torch.sqrt(torch.clamp(1 - z * z, min=0))
            phi = float(LC.TAU32) * s1
            m = torch.stack([q * torch.cos(phi), q * torch.sin(phi), z], -1)
            y = o + a[0] * m
            w = float((LC.FOURPI32 * c.lights[k][4]) * c.lights[k][4])
        d = y - x[:, None, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        nd = (n[:, None, 0] * d[..., 0] + n[:, None, 1] * d[..., 1]) + n[:, None, 2] * d[..., 2]
        md = -((m[..., 0] * d[..., 0] + m[..., 1] * d[..., 1]) + m[..., 2] * d[..., 2])
        g = (nd * md) / (dd * dd)
        g = torch.where((nd > 0) & (md > 0) & (dd > 0) & torch.isfinite(g), g, torch.zeros_like(g))
        _, t, pid, _ = sc.trace_shade(x[:, None, :].expand_as(d).reshape(-1, 3), d.reshape(-1, 3), t_min=0.0, return_hits=True)
        vis = ~((pid >= 0) & (t < c.t_max)).reshape(g.shape)
        acc = torch.zeros(len(L), device="cuda")
        for i in range(c.S):
            acc = torch.where(vis[:, i], acc + g[:, i], acc)
        out[k, L] = (acc * w) / float(c.S)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["room_quad", "room_sphere"])
def test_against_torch_built_rays_and_trace_shade(tx, name):
    from conftest import rel_l2
    c = LC.case(name)
    F, _ = run(tx, c)
    want = torch_route(scene_of(tx, c.geo), c)
    tex = c.ref().tex
    err = rel_l2(F[:, tex], want[:, tex])
    print("irt_lights %s against torch rays + trace_shade + torch reduction: relative L2 %.3e; bits %s" % (name, err, "agree" if np.array_equal(F[:, tex], want[:, tex]) else "differ"))
    assert np.abs(want[:, tex]).max() > 0 and err <= 1e-3


# ---- 4. purity -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_result_is_a_pure_function_of_the_inputs(tx):
    from texir_code_amd import _lib
    c = LC.case("list200")
    sc = scene_of(tx, c.geo)
    base, st = run(tx, c)
    tex = c.ref().tex
    unlisted = np.setdiff1d(np.arange(c.Nt), tex)
    assert (base[:, unlisted] == LC.SENTINEL).all() and np.isfinite(base).all() and (base[:, tex] != LC.SENTINEL).all()
    again, st2 = run(tx, c)
    assert np.array_equal(base, again) and np.array_equal(st, st2), "second run"
    perm = np.random.default_rng(3).permutation(len(c.ids))
    assert np.array_equal(base, run(tx, c, ids=c.ids[perm])[0]), "shuffled list"
    assert np.array_equal(base, run(tx, c, ids=np.concatenate([c.ids, c.ids[:70], [-5, c.Nt, 2 ** 31 - 1]]))[0]), "duplicates and ids outside the atlas"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run(tx, c)[0]
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(base, on_side), "side stream"
    # a captured graph replayed twice, on caller-owned buffers with guard words behind F; the light records live on the device and are moved between replays
    L = _lib.lib()
    pos, nrm, shift = (torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.shift))
    ids = torch.from_numpy(c.ids).cuda()
    lights = torch.from_numpy(c.lights).cuda()
    Kl, Nt, guard = c.K, c.Nt, 64
    out = torch.full((Kl * Nt + guard,), LC.SENTINEL, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_irt_lights(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), ids.numel(), Nt, _lib.ptr(lights), Kl, c.S, c.t_max,
                                          _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(LC.SENTINEL)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(base, out[:Kl * Nt].reshape(Kl, Nt).cpu().numpy()), "graph replay"
        assert np.array_equal(st, stats.cpu().numpy()), "stats of a replay"
        assert (out[Kl * Nt:] == LC.SENTINEL).all(), "guard words"
    moved = c.lights.copy()
    moved[0, 1:4] += np.array([0.5, -0.25, 0.75], np.float32)
    moved[1, 1:4] += np.array([-1.0, 0.125, 0.5], np.float32)
    lights.copy_(torch.from_numpy(moved))
    out.fill_(LC.SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    direct = run(tx, c, lights=moved)[0]
    assert not np.array_equal(direct, base)
    assert np.array_equal(direct, out[:Kl * Nt].reshape(Kl, Nt).cpu().numpy()), "replay with moved lights"
    assert (out[Kl * Nt:] == LC.SENTINEL).all(), "guard words"


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise_and_empty_calls_write_nothing(tx):
    from texir_code_amd import _lib
    c = LC.case("list65")
    sc = scene_of(tx, c.geo)
    pos, nrm, shift = (torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.shift))
    ids = torch.from_numpy(c.ids).cuda()
    lights = torch.from_numpy(c.lights).cuda()
    with pytest.raises(_lib.TexirError, match="K must be in 0..8"):
        sc.irt_lights(pos, nrm, shift, torch.zeros((9, 16)), 16, texel_ids=ids)
    for bad_s in (0, -1, 65537):
        with pytest.raises(_lib.TexirError, match="S must be in 1..65536"):
            sc.irt_lights(pos, nrm, shift, lights, bad_s, texel_ids=ids)
    for bad_t in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.TexirError, match="t_max must be finite"):
            sc.irt_lights(pos, nrm, shift, lights, 16, texel_ids=ids, t_max=bad_t)
    with pytest.raises(ValueError):
        sc.irt_lights(pos, nrm, shift, torch.zeros((2, 15)), 16, texel_ids=ids)
    L = _lib.lib()
    Nt = c.Nt
    out = torch.full((c.K, Nt), LC.SENTINEL, device="cuda")
    P = _lib.ptr

    def call(K=c.K, S=16, t_max=0.999, n_ids=ids.numel(), nt=Nt, pos_=pos, nrm_=nrm, shift_=shift, lights_=lights, out_=out, ids_=ids, scene=sc.h):
        return L.texir_irt_lights(scene, P(pos_), P(nrm_), P(shift_), P(ids_), n_ids, nt, P(lights_), K, S, t_max, P(out_), None, _lib.stream_ptr())
    for kw in (dict(pos_=None), dict(nrm_=None), dict(shift_=None), dict(lights_=None), dict(out_=None), dict(scene=None)):
        with pytest.raises(_lib.TexirError, match="null argument"):
            _lib.check(call(**kw))
    with pytest.raises(_lib.TexirError, match="K must be in 0..8"):        # a bad K is reported before any null buffer
        _lib.check(call(K=9, lights_=None, out_=None))
    with pytest.raises(_lib.TexirError, match="K must be in 0..8"):
        _lib.check(call(K=-1, lights_=None, out_=None))
    with pytest.raises(_lib.TexirError, match="negative"):
        _lib.check(call(n_ids=-1))
    with pytest.raises(_lib.TexirError, match="negative"):
        _lib.check(call(nt=-1, ids_=None))
    _lib.check(call(K=0, lights_=None, out_=None))                        # no light: nothing to do, whatever the buffers
    _lib.check(call(K=0))
    _lib.check(call(n_ids=0))                                              # an empty list
    torch.cuda.synchronize()
    assert (out == LC.SENTINEL).all()
    F0 = sc.irt_lights(pos, nrm, shift, torch.zeros((0, 16)), 16, texel_ids=ids)
    assert tuple(F0.shape) == (0, Nt)
    F, st = sc.irt_lights(pos, nrm, shift, lights, 16, texel_ids=ids[:0], out=out, stats=True)
    torch.cuda.synchronize()
    assert F is out and (out == LC.SENTINEL).all() and not st.any()


# ---- 6. linearity end to end -------------------------------------------------------------------------------------------------------------------------------------------

def test_add_with_two_colours_is_the_sum_of_two_one_light_calls(tx):
    from texir_code_amd import irtlight
    c = LC.case("list200")
    tex = c.ref().tex
    both = run(tx, c)[0][:, tex]
    one = [run(tx, c, lights=c.lights[k:k + 1])[0][:, tex] for k in range(2)]
    assert np.array_equal(both[0], one[0][0]) and np.array_equal(both[1], one[1][0])
    E = np.random.default_rng(7).random((len(tex), 3), dtype=np.float32)
    cols = [(3.0, 2.5, 2.0), (0.5, 8.0, 1.0)]
    got = irtlight.add(E, both, cols)
    want = irtlight.add(irtlight.add(E, one[0], cols[:1]), one[1], cols[1:])
    assert got.dtype == np.float32 and np.array_equal(got, want) and (got != E).any()
    gt = irtlight.add(torch.from_numpy(E).cuda(), torch.from_numpy(both).cuda(), cols)
    assert np.array_equal(gt.cpu().numpy(), got)


# ---- 7. the stage and the command ------------------------------------------------------------------------------------------------------------------------------------

def test_stage_writes_the_light_files_and_light_irt_round_trips(tmp_path, capsys):
    from texir_code_amd import datasets as D, io_formats as IO, tools
    from texir_code_amd.trainer import exp_runner as ER

    def stage(tag, extra):
        root = str(tmp_path / tag)
        D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
        conf = str(tmp_path / (tag + ".conf"))
        D.write_conf(conf, root, cube_res=16, spp=(64, 16), model="irt")
        if extra:
            txt = open(conf).read()
            assert "batch_size = 1" in txt
            with open(conf, "w") as f:
                f.write(txt.replace("batch_size = 1", "batch_size = 1\n    " + "\n    ".join(extra), 1))
        d = os.path.join(root, "vrproc", "hdr_texture")
        before = set(os.listdir(d))
        ER.main(["--conf", conf, "--trainstage", "IrrT", "--gpu", "0"])
        return root, d, {f: open(os.path.join(d, f), "rb").read() for f in sorted(set(os.listdir(d)) - before)}

    _, d0, plain = stage("plain", [])
    _, d1, none = stage("none", ["irt_lights = none"])
    # the lights: a ceiling panel and a sphere placed from the mesh's own bounds
    verts = np.array([[float(v) for v in l.split()[1:4]] for l in open(os.path.join(d0, "out1.obj")) if l.startswith("v ")])
    lo, hi = verts.min(0), verts.max(0)
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.15 * ext[0], 0, 0], [0, 0, 0.15 * ext[2]]
    spec = {"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                       {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.05 * float(ext.min())}]}
    js = str(tmp_path / "lights.json")
    with open(js, "w") as f:
        json.dump(spec, f)
    _, d2, lit = stage("lights", ['irt_lights = "%s"' % js, "irt_light_samples = 16"])
    # without the key and with `none`: the same files, byte for byte; with lights: the light files and nothing else, every other file byte for byte
    assert "0_irr_texture.hdr" in plain and sorted(none) == sorted(plain) and all(none[f] == plain[f] for f in plain)
    assert sorted(set(lit) - set(plain)) == ["0_irr_texture_light0.hdr", "0_irr_texture_light1.hdr"]
    assert all(lit[f] == plain[f] for f in plain)
    full = IO.read_hdr(os.path.join(d2, "0_irr_texture.hdr")).astype(np.float64)
    F = [IO.read_hdr(os.path.join(d2, "0_irr_texture_light%d.hdr" % k)).astype(np.float64) for k in (0, 1)]
    for k in (0, 1):
        assert F[k].shape == full.shape and F[k].max() > 0 and (F[k][..., 0] == F[k][..., 1]).all() and (F[k][..., 0] == F[k][..., 2]).all()
        with capsys.disabled():
            print("stage: light %d reaches %.1f %% of the atlas, largest factor %.4f" % (k, 100.0 * (F[k][..., 0] > 0).mean(), F[k].max()))
    assert tools.main(["light-irt", d2, "--light", "0", "--colour", "20,18,15", "--light", "1", "--colour", "5,5,9"]) == 0
    got = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    want = full + F[0] * np.array([20.0, 18.0, 15.0]) + F[1] * np.array([5.0, 5.0, 9.0])
    # an RGBE pixel keeps 8 bits below its largest channel's power of two
    assert (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    assert tools.main(["light-irt", d2, "--light", "0", "--colour", "1,1,1"]) == 1            # refuses to overwrite
    assert tools.main(["light-irt", d0, "--light", "0", "--colour", "1,1,1"]) == 1            # no light files there
    assert "0_irr_texture_light0.hdr" in capsys.readouterr().out
