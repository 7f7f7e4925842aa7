"""trace_occluded (csrc/device_common.h), trace_occluded_kernel (csrc/occlusion.hip) behind texir_trace_occluded / Scene.test_occlusions, and the any-hit forms
of the light pass and the bake (texir_irt_lights_any, texir_atlas_bake_any; query="any"; train.irt_light_query; bake-atlas --query).

  1. reference   every certain ray of every case and segment of occlusion_cases gets its answer (test_occlusion_ref_cpu.py proves the caps and the checker);
                 stats[0] is the sum of the output; ray counts 1 .. 1000 (ragged waves, the block edge, a lane alone in its wave);
  2. identity    at t_near = 0 the answer is `hit & (t_hit < t_far)` of trace_shade(t_min=0, return_hits=True) on EVERY ray of every case (the tie case
                 included), on the 4-wide tree, the binary tree and the deeper tree of TEXIR_MAX_LEAF=1; one wave in which the lanes that hit finish with
                 entries in the private overflow part of their stacks while the other lanes walk on;
  3. same bits   query="any" returns the bits of query="closest": F and stats of every light case, view / pix / rgb / stats of every bake case, and both
                 pass the modules' own float64 checks;
  4. house rules guard bytes, a side stream, a second run, a captured graph replayed twice, moved lights between replays, R = 0, null pointers, t_far = nan;
  5. stage       train.irt_light_query = any and bake-atlas --query any write the files of the defaults, byte for byte.

The overflow case of 2 is built, not counted (the occlusion kernel has no counting instantiation): 3000 stacked triangles under TEXIR_MAX_LEAF=1 are a 4-wide
tree at least six levels deep in which a ray along the stack's axis enters every child of every node it visits -- three pushes per level, more than the
12 LDS entries of a lane before its first leaf.

Run on an MI355X: 101 passed in 21 s (the float64 lists of the four 20 000-triangle cases, about 3 s each, included).
"""
import os

import numpy as np
import pytest
import torch

import atlas_bake_cases as AB
import light_cases as LC
import occlusion_cases as OC

pytestmark = pytest.mark.gpu

_SC = {}


def scene_of(tx, geo, tag=""):
    key = (geo.name, tag)
    if key not in _SC:
        _SC[key] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    return _SC[key]


def occluded(sc, org, dir, t_near, t_far):
    got, st = sc.test_occlusions(torch.from_numpy(org), torch.from_numpy(dir), t_near, t_far, stats=True)
    assert got.dtype == torch.bool and tuple(got.shape) == (org.reshape(-1, 3).shape[0],)
    got = got.cpu().numpy()
    assert int(st[0]) == int(got.sum()), "stats[0] is the number of occluded rays"
    return got


def closest(sc, org, dir):
    _, t, pid, _ = sc.trace_shade(torch.from_numpy(org), torch.from_numpy(dir), t_min=0.0, return_hits=True)
    return t.cpu().numpy(), pid.cpu().numpy().astype(np.int64)


def identity(sc, c, what):
    t, pid = closest(sc, c.org, c.dir)
    for tag, tn, tf in (c.equal_segments() if c.name != "tie" else [("tie", 0.0, OC.TIE_FAR)]):
        OC.equals_closest(occluded(sc, c.org, c.dir, 0.0, tf), t, pid, tf, "%s %s %s" % (c.name, tag, what))


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", OC.NAMES)
def test_every_certain_ray_gets_its_answer(tx, name):
    c = OC.case(name)
    sc = scene_of(tx, c.geo)
    for tag, tn, tf in c.segments():
        got = occluded(sc, c.org, c.dir, tn, tf)
        unc = OC.check_certain(*c.classify(tn, tf), got, "%s %s" % (name, tag))
        print("occlusion %-20s %-12s: %d of %d occluded, %d uncertain" % (name, tag, got.sum(), c.R, unc))
    if name == "grid_zero_nonfinite":
        assert not any(occluded(sc, c.org, c.dir, tn, tf).any() for _, tn, tf in c.segments())


@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_ray_counts(tx, R):
    c = OC.case("room_random")
    sc = scene_of(tx, c.geo)
    pick = np.arange(7, 7 + R) % c.R
    org, dir = np.ascontiguousarray(c.org[pick]), np.ascontiguousarray(c.dir[pick])
    t, pid = closest(sc, org, dir)
    for tag, tn, tf in c.segments():
        got = occluded(sc, org, dir, tn, tf)
        occ, vis = c.classify(tn, tf)
        OC.check_certain(occ[pick], vis[pick], got, "room_random[%d] %s" % (R, tag))
        if tn == 0.0:
            OC.equals_closest(got, t, pid, tf, "room_random[%d] %s" % (R, tag))


# ---- 2. the identity with the closest-hit query ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", OC.NAMES + ("tie",))
def test_equals_the_closest_hit_answer_on_every_ray(tx, name):
    c = OC.case(name)
    identity(scene_of(tx, c.geo), c, "4-wide")


@pytest.mark.parametrize("var,value", [("TEXIR_BVH_WIDTH", "2"), ("TEXIR_MAX_LEAF", "1")])
@pytest.mark.parametrize("name", OC.NAMES + ("tie",))
def test_equals_the_closest_hit_answer_on_other_trees(tx, monkeypatch, name, var, value):
    monkeypatch.setenv(var, value)
    c = OC.case(name)
    sc = tx.Scene(c.geo.verts, c.geo.tris, c.geo.tri_uvs, c.geo.hdr)          # built under the switch, kept out of the shared cache
    identity(sc, c, "%s=%s" % (var, value))
    for tag, tn, tf in c.segments():
        OC.check_certain(*c.classify(tn, tf), occluded(sc, c.org, c.dir, tn, tf), "%s %s %s=%s" % (name, tag, var, value))


def test_a_lane_with_overflow_entries_finishes_by_a_hit_and_the_wave_goes_on(tx, monkeypatch):
    """the 3000 stacked triangles, one triangle per leaf: rays along +z from below the stack.  Even lanes pass through the triangles' interior (occluded at
    the first leaf, with the far children of every level above it on their stacks: beyond the LDS part); odd lanes pass through every box beside the
    triangles (x + y > 1) and walk all of them to the end"""
    monkeypatch.setenv("TEXIR_MAX_LEAF", "1")
    geo = OC.case("patho_stack").geo
    sc = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    assert sc.info()["max_depth"] >= 5, sc.info()
    n = 192
    k = np.arange(n)
    hit = k % 2 == 0
    xy = np.where(hit[:, None], np.stack([0.125 + 0.25 * (k % 3) / 3, 0.125 + 0.25 * (k % 5) / 5], 1), np.stack([0.625 + 0.25 * (k % 3) / 3, 0.625 + 0.25 * (k % 5) / 5], 1))
    org = np.concatenate([xy, np.full((n, 1), -1.0)], 1).astype(np.float32)
    dir = np.tile(np.array([[0, 0, 8]], np.float32), (n, 1))
    t, pid = closest(sc, org, dir)
    assert (pid[hit] >= 0).all() and (pid[~hit] == -1).all()
    for tf in (float("inf"), 1.0, 0.25, 0.0625):                           # (the stack spans t in [0.125, 0.5])
        got = occluded(sc, org, dir, 0.0, tf)
        OC.equals_closest(got, t, pid, tf, "stack overflow t_far %r" % tf)
        assert got[hit].all() == (tf > 0.125) and not got[~hit].any()
    # behind the first 1000 triangles: the lanes that hit still hit, later
    assert np.array_equal(occluded(sc, org, dir, 0.25, float("inf")), hit)
    assert not occluded(sc, org, dir, 0.51, float("inf")).any()


# ---- 3. query="any" returns the bits of query="closest" --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LC.ALL)
def test_lights_any_returns_the_bits_of_closest(tx, name):
    import test_gpu_irt_lights as TL
    c = LC.case(name)
    F0, s0 = TL.run(tx, c)
    F1, s1 = TL.run(tx, c, query="any")
    assert np.array_equal(F0.view(np.uint32), F1.view(np.uint32)) and np.array_equal(s0, s1), name
    for F, st in ((F0, s0), (F1, s1)):
        fails, _ = LC.check(c, F, st, LC.SENTINEL)
        assert not fails, fails
    if name == "closed_box":
        assert not F1.any() and s1[0] > 0 and s1[1] == 0
    if name == "on_surface":
        assert c.t_max == np.float32(0.999) and s1[1] == s1[0] > 0 and (F1 > 0).any()


@pytest.mark.parametrize("name", AB.ALL)
def test_bake_any_returns_the_bits_of_closest(tx, name):
    from texir_code_amd import atlas
    case = AB.case(name)
    sc = scene_of(tx, case.geo)
    sent = (-7, 5, 0.25)

    def run(query):
        out = (torch.full((case.Nt,), sent[0], device="cuda", dtype=torch.int32), torch.full((case.Nt, 2), sent[1], device="cuda", dtype=torch.int32),
               torch.full((case.Nt, 3), sent[2], device="cuda", dtype=torch.float32))
        res = atlas.bake_atlas(sc, torch.from_numpy(case.pos), torch.from_numpy(case.nrm), torch.from_numpy(case.Wm), torch.from_numpy(case.cam),
                               torch.from_numpy(case.panos()), None if case.valid is None else torch.from_numpy(case.valid), case.cos_min,
                               None if case.ids is None else torch.from_numpy(np.ascontiguousarray(case.ids, np.int32)), out=out, stats=True, query=query)
        return [r.cpu().numpy() for r in res]
    a, b = run("closest"), run("any")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3], b[3]), name
    for view, pix, rgb, _ in (a, b):
        fails = AB.check(case, view, pix, rgb, sentinel=sent)
        assert not fails, (len(fails), fails[:5])


# ---- 4. house rules --------------------------------------------------------------------------------------------------------------------------------------------

def test_pure_function_guard_bytes_streams_and_graph_replays(tx):
    from texir_code_amd import _lib
    c = OC.case("house_random")
    sc = scene_of(tx, c.geo)
    _, tn, tf = c.segments()[2]
    base = occluded(sc, c.org, c.dir, tn, tf)
    assert 0 < base.sum() < c.R
    assert np.array_equal(base, occluded(sc, c.org, c.dir, tn, tf)), "second run"
    # any leading shape, an out buffer of either byte type
    o3, d3 = torch.from_numpy(c.org).reshape(4, -1, 3), torch.from_numpy(c.dir).reshape(4, -1, 3)
    out8 = torch.full((c.R,), 9, dtype=torch.uint8, device="cuda")
    assert sc.test_occlusions(o3, d3, tn, tf, out=out8) is out8 and np.array_equal(out8.cpu().numpy(), base.astype(np.uint8))
    with pytest.raises(ValueError):
        sc.test_occlusions(o3, d3, tn, tf, out=torch.zeros(c.R + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        sc.test_occlusions(o3, d3, tn, tf, out=torch.zeros(c.R, dtype=torch.int32, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = occluded(sc, c.org, c.dir, tn, tf)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(base, on_side), "side stream"
    # a captured graph on caller-owned buffers with guard bytes behind the output, an odd ray count
    L = _lib.lib()
    R, guard = c.R - 3, 67
    org, dir = torch.from_numpy(c.org).cuda(), torch.from_numpy(c.dir).cuda()
    out = torch.full((R + guard,), 7, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_trace_occluded(sc.h, _lib.ptr(org), _lib.ptr(dir), R, tn, tf, _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(7)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[:R].cpu().numpy(), base[:R].astype(np.uint8)), "graph replay"
        assert int(stats[0]) == int(base[:R].sum()) and (out[R:] == 7).all(), "stats and guard bytes of a replay"


def test_lights_any_replays_with_moved_lights(tx):
    import test_gpu_irt_lights as TL
    from texir_code_amd import _lib
    c = LC.case("list200")
    sc = TL.scene_of(tx, c.geo)
    base, st = TL.run(tx, c)
    L = _lib.lib()
    pos, nrm, shift = (torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.shift))
    ids = torch.from_numpy(c.ids).cuda()
    lights = torch.from_numpy(c.lights).cuda()
    Kl, Nt, guard = c.K, c.Nt, 64
    out = torch.full((Kl * Nt + guard,), LC.SENTINEL, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_irt_lights_any(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), ids.numel(), Nt, _lib.ptr(lights), Kl, c.S, c.t_max,
                                              _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(LC.SENTINEL)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(base, out[:Kl * Nt].reshape(Kl, Nt).cpu().numpy()) and np.array_equal(st, stats.cpu().numpy()), "graph replay"
        assert (out[Kl * Nt:] == LC.SENTINEL).all(), "guard words"
    moved = c.lights.copy()
    moved[0, 1:4] += np.array([0.5, -0.25, 0.75], np.float32)
    moved[1, 1:4] += np.array([-1.0, 0.125, 0.5], np.float32)
    lights.copy_(torch.from_numpy(moved))
    out.fill_(LC.SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    direct = TL.run(tx, c, lights=moved)[0]                                # (the closest-hit call with the moved lights)
    assert not np.array_equal(direct, base)
    assert np.array_equal(direct, out[:Kl * Nt].reshape(Kl, Nt).cpu().numpy()), "replay with moved lights"
    assert (out[Kl * Nt:] == LC.SENTINEL).all(), "guard words"


def test_empty_null_and_nan_arguments(tx):
    from texir_code_amd import _lib
    c = OC.case("box_random")
    sc = scene_of(tx, c.geo)
    L = _lib.lib()
    P = _lib.ptr
    org, dir = torch.from_numpy(c.org).cuda(), torch.from_numpy(c.dir).cuda()
    out = torch.full((c.R,), 5, dtype=torch.uint8, device="cuda")

    def call(R=c.R, tn=0.0, tf=1.0, org_=org, dir_=dir, out_=out, scene=sc.h):
        return L.texir_trace_occluded(scene, P(org_), P(dir_), R, tn, tf, P(out_), None, _lib.stream_ptr())
    for kw in (dict(org_=None), dict(dir_=None), dict(out_=None), dict(scene=None)):
        with pytest.raises(_lib.TexirError, match="null argument"):
            _lib.check(call(**kw))
    with pytest.raises(_lib.TexirError, match="negative ray count"):
        _lib.check(call(R=-1))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.TexirError, match="t_near must be finite and >= 0"):
            _lib.check(call(tn=bad))
    _lib.check(call(R=0))
    _lib.check(call(R=0, org_=None, dir_=None, out_=None))                 # no ray: nothing to do, whatever the buffers
    torch.cuda.synchronize()
    assert (out == 5).all()
    # a segment that holds no t: every ray is written, none is occluded
    for tn, tf in ((0.0, float("nan")), (0.5, 0.5), (0.75, 0.25), (0.0, 0.0), (0.0, -1.0), (0.0, -float("inf"))):
        out.fill_(5)
        _lib.check(call(tn=tn, tf=tf))
        torch.cuda.synchronize()
        assert (out == 0).all(), (tn, tf)
    assert occluded(sc, c.org, c.dir, 0.0, float("inf")).all()             # (from inside the closed box every ray is occluded somewhere)
    e = sc.test_occlusions(torch.zeros((0, 3)), torch.zeros((0, 3)))
    assert tuple(e.shape) == (0,) and e.dtype == torch.bool
    # the shadowed calls' argument rules hold for the _any calls, under their own names
    with pytest.raises(_lib.TexirError, match="texir_irt_lights_any: K must be in 0..8"):
        _lib.check(L.texir_irt_lights_any(sc.h, None, None, None, None, 0, 4, None, 9, 16, 0.999, None, None, _lib.stream_ptr()))
    with pytest.raises(_lib.TexirError, match="texir_atlas_bake_any: null argument"):
        _lib.check(L.texir_atlas_bake_any(sc.h, None, None, None, 0, 4, None, None, None, None, 1, 4, 8, 0.1, None, None, None, None, _lib.stream_ptr()))
    with pytest.raises(ValueError):
        sc.irt_lights(torch.zeros((4, 3)), torch.zeros((4, 3)), torch.zeros((4, 2)), torch.zeros((1, 16)), 16, query="first")


# ---- 5. the stage and the command ------------------------------------------------------------------------------------------------------------------------------

def test_stage_key_writes_the_files_of_the_default(tmp_path):
    import json
    from texir_code_amd import datasets as D
    from texir_code_amd.trainer import exp_runner as ER

    def stage(tag, extra, js=None):
        root = str(tmp_path / tag)
        D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
        d = os.path.join(root, "vrproc", "hdr_texture")
        if js is None:
            verts = np.array([[float(v) for v in l.split()[1:4]] for l in open(os.path.join(d, "out1.obj")) if l.startswith("v ")])
            lo, hi = verts.min(0), verts.max(0)
            ext, ctr = hi - lo, (hi + lo) / 2
            a, b = [0.15 * ext[0], 0, 0], [0, 0, 0.15 * ext[2]]
            spec = {"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                               {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.05 * float(ext.min())}]}
            js = str(tmp_path / "lights.json")
            with open(js, "w") as f:
                json.dump(spec, f)
        conf = str(tmp_path / (tag + ".conf"))
        D.write_conf(conf, root, cube_res=16, spp=(64, 16), model="irt")
        txt = open(conf).read()
        assert "batch_size = 1" in txt
        with open(conf, "w") as f:
            f.write(txt.replace("batch_size = 1", "batch_size = 1\n    " + "\n    ".join(['irt_lights = "%s"' % js, "irt_light_samples = 16"] + extra), 1))
        before = set(os.listdir(d))
        ER.main(["--conf", conf, "--trainstage", "IrrT", "--gpu", "0"])
        return js, {f: open(os.path.join(d, f), "rb").read() for f in sorted(set(os.listdir(d)) - before)}
    js, plain = stage("plain", [])
    _, closest_ = stage("closest", ["irt_light_query = closest"], js)
    _, any_ = stage("any", ["irt_light_query = any"], js)
    assert "0_irr_texture_light0.hdr" in plain and "0_irr_texture_light1.hdr" in plain
    for other in (closest_, any_):
        assert sorted(other) == sorted(plain) and all(other[f] == plain[f] for f in plain)


def test_bake_command_writes_the_files_of_the_default(tx, tmp_path):
    from texir_code_amd import atlas, datasets as D, io_formats as IO, tools
    root = str(tmp_path / "data")
    s = D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
    E = atlas.read_extrinsics(root)
    ids = [l.strip() for l in open(os.path.join(root, "info", "aligned.txt")) if l.strip()]
    lit = tx.Scene(s["verts"], s["tris"], s["tri_uvs"], s["hdr"], device=0)
    traced = atlas.trace_panoramas(lit, E, 50, 100).cpu().numpy()
    for k, i in enumerate(ids):
        os.makedirs(os.path.join(root, "hdr", i))
        IO.write_hdr(os.path.join(root, "hdr", i, "ccm.hdr"), traced[k])
    dirs = {q: str(tmp_path / q) for q in ("default", "closest", "any")}
    assert tools.main(["bake-atlas", root, "64", "--out", dirs["default"]]) == 0
    assert tools.main(["bake-atlas", root, "64", "--out", dirs["closest"], "--query", "closest"]) == 0
    assert tools.main(["bake-atlas", root, "64", "--out", dirs["any"], "--query=any"]) == 0
    files = sorted(os.listdir(dirs["default"]))
    assert "hdr_texture.hdr" in files and "0.png" in files
    for q in ("closest", "any"):
        assert sorted(os.listdir(dirs[q])) == files
        for f in files:
            assert open(os.path.join(dirs[q], f), "rb").read() == open(os.path.join(dirs["default"], f), "rb").read(), (q, f)
