"""irt_lights_mesh_kernel (csrc/irtlightmesh.hip) and spec_lights_mesh_kernel (csrc/speclightmesh.hip) behind texir_irt_lights_mesh, texir_spec_lights_mesh,
Scene.irt_lights / spec_lights(occluders=...), the IrT stage's train.irt_light_objects, `light-irt --objects` and the evaluation model's test.objects.

  1. intervals   every case of light_mesh_cases inside its float64 reference, stats inside its counts, unlisted texels untouched: F, and R in a second
                 parametrisation;
  2. identities  J = 0, every matrix non-finite, objects far from every segment: the bits of irt_lights / spec_lights for query = closest and any, F, R and
                 stats alike;
  3. prefilter   prefilter=False returns the same bits on every case (inside test 1);
  4. one sample  quad lights at S = 1: F_mesh == where(blocked, 0, F_plain) bit for bit, blocked = the OR over instances of the occluder's own
                 test_occlusions on the restated object-space ray;
  5. restatement general S: F against lights_mesh_f32 with the GPU's own occlusion answers;
  6. monotone    F_mesh <= F and R_mesh <= R per value; the enclosed light gives exactly +0 and no visible sample;
  7. purity      second run, shuffled list, duplicates and ids outside the atlas, a side stream, a recorded graph replayed after the matrices moved;
  8. errors      every refused argument raises with the header's text; empty calls write nothing;
  9. poses       host poses and the device [J,12] form give the same bits; a singular pose is a ValueError;
 10. end to end  the stage's files with train.irt_light_objects, light-irt --objects; byte-identical files without the key;
 11. model       lit_model with test.objects equals add_view of direct calls with the objects; none leaves render() as it is.
"""
import json
import os

import numpy as np
import pytest
import torch

import irt_shadow_mesh_cases as MC
import light_cases as LC
import light_mesh_cases as LM
import spec_light_cases as SL

pytestmark = pytest.mark.gpu

SENTINEL = LM.SENTINEL
_SC, _OCC = {}, {}


def scene_of(tx, geo):
    if geo.name not in _SC:
        _SC[geo.name] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    return _SC[geo.name]


def occluder_of(tx, name):
    if name not in _OCC:
        g = MC.occluder(name)
        _OCC[name] = tx.Scene.occluder(g.verts, g.tris)
    return _OCC[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def objects_of(tx, c, w2o=None):
    """the case's objects as keywords: the DEVICE world-to-object matrices"""
    return dict(occluders=[occluder_of(tx, n) for n in c.occ], instances=c.inst, poses=dev(c.w2o) if w2o is None else w2o)


def run(tx, c, objects=True, ids="case", lights=None, w2o=None, **kw):
    """-> (F [K,Nt] or R [K,P] numpy, stats [2] numpy) with the sentinel wherever the call does not write; objects=False: the plain call"""
    sc = scene_of(tx, c.geo)
    lights = c.lights if lights is None else lights
    out = torch.full((lights.shape[0], c.Nt), SENTINEL, device="cuda")
    ids = c.ids if isinstance(ids, str) else ids
    ids = None if ids is None else dev(np.asarray(ids, np.int32))
    if objects:
        kw.update(objects_of(tx, c, w2o))
    if isinstance(c, SL.Case):
        got, st = sc.spec_lights(dev(c.pos), dev(c.nrm), dev(c.rough), dev(c.shift), dev(c.cam), torch.from_numpy(lights), c.S, texel_ids=ids, t_max=c.t_max,
                                 clamp_eps=c.ceps, out=out, stats=True, **kw)
    else:
        got, st = sc.irt_lights(dev(c.pos), dev(c.nrm), dev(c.shift), torch.from_numpy(lights), c.S, texel_ids=ids, t_max=c.t_max, out=out, stats=True, **kw)
    assert got is out
    return out.cpu().numpy(), st.cpu().numpy()


# ---- 1. intervals, 3. the prefilter ----------------------------------------------------------------------------------------------------------------------------------

def inside(tx, c, what):
    got, st = run(tx, c)
    fails, worst = LM.check(c, got, st, SENTINEL)
    print("%s %-16s S=%-3d K=%d J=%d: worst share of an interval %.3f; stats %s inside %s" % (what, c.name, c.S, c.K, c.J, worst, st.tolist(), c.ref().counts()))
    assert not fails, "\n".join(fails)
    assert (got[:, c.ref().tex] != SENTINEL).all(), "a listed texel was not written"
    off, st_off = run(tx, c, prefilter=False)
    assert np.array_equal(bits(got), bits(off)) and st.tolist() == st_off.tolist(), "the prefilter changes a bit"
    return got, st


@pytest.mark.parametrize("name", LM.ALL)
def test_every_listed_texel_inside_the_float64_reference(tx, name):
    inside(tx, LM.case(name), "irt_lights_mesh")


@pytest.mark.parametrize("name", LM.SPEC_ALL)
def test_every_listed_pixel_inside_the_float64_reference(tx, name):
    inside(tx, LM.spec_case(name), "spec_lights_mesh")


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LM.IDENTITIES + tuple("spec:" + n for n in LM.SPEC_IDENTITIES))
def test_objects_that_block_nothing_return_the_bits_of_the_plain_pass(tx, name):
    c = LM.spec_case(name[5:]) if name.startswith("spec:") else LM.case(name)
    got, st = run(tx, c)
    assert (got[:, c.ref().tex] > 0).any()
    for query in ("closest", "any"):
        plain, st0 = run(tx, c, objects=False, query=query)
        assert np.array_equal(bits(got), bits(plain)), "%s: values differ from query=%s" % (name, query)
        assert st.tolist() == st0.tolist(), "%s: stats differ from query=%s" % (name, query)
    # with occluders `query` is accepted and ignored
    assert np.array_equal(bits(got), bits(run(tx, c, query="any")[0]))


# ---- 4. one-sample exactness -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", LM.ONE_SAMPLE)
def test_one_sample_is_the_plain_factor_or_zero_by_the_occluders_own_query(tx, name):
    """S = 1, quad lights: d is IEEE arithmetic on exact float32 values, so numpy restates it bit for bit; the transform, the range (0, t_max) and the union
    are pinned to the existing occlusion query"""
    c = LM.case(name)
    assert c.S == 1 and all(LC.record_kind(r) == "quad" for r in c.lights)
    got, st = run(tx, c)
    plain, st0 = run(tx, c, objects=False, query="any")
    L = c.ref().tex
    s0, s1 = LC.sample_points(c.shift[L], 1)
    x = c.pos[L]
    n_blocked = 0
    for k in range(c.K):
        o, a, b = c.lights[k][1:4], c.lights[k][4:7], c.lights[k][7:10]
        y = np.stack([(o[i] + s0[:, 0] * a[i]) + s1[:, 0] * b[i] for i in range(3)], 1).astype(np.float32)
        d = (y - x).astype(np.float32)
        blocked = np.zeros(len(L), bool)
        for j in range(c.J):
            occ = occluder_of(tx, c.occ[c.inst[j]])
            blocked |= occ.test_occlusions(dev(MC.point_f32(c.w2o[j], x)), dev(MC.dir_f32(c.w2o[j], d)), 0.0, c.t_max).cpu().numpy().astype(bool)
        want = np.where(blocked, np.float32(0), plain[k, L])
        assert np.array_equal(bits(got[k, L]), bits(want)), "light %d: %d of %d texels differ" % (k, int((bits(got[k, L]) != bits(want)).sum()), len(L))
        n_blocked += int((blocked & (plain[k, L] > 0)).sum())
    print("irt_lights_mesh %s: %d lit texels blocked by an object; stats %s, plain %s" % (name, n_blocked, st.tolist(), st0.tolist()))
    assert n_blocked > 0 and st[0] == st0[0] and st[1] == st0[1] - n_blocked


# ---- 5. the restatement with the GPU's own occlusion answers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("tri", "cube", "twice", "s24", "null", "behind_light", "inside_box"))
def test_agrees_with_the_float32_restatement(tx, name):
    c = LM.case(name)
    sc = scene_of(tx, c.geo)
    F, st = run(tx, c)

    def scene(o, d):                                                              # (t, pid) of a closest hit that says what the scene's occlusion query says
        hit = sc.test_occlusions(dev(o), dev(d), 0.0, c.t_max).cpu().numpy().astype(bool)
        return np.where(hit, np.float32(0), np.float32(np.inf)), np.where(hit, 0, -1)

    def inst(j, o, d, t_max):
        return occluder_of(tx, c.occ[c.inst[j]]).test_occlusions(dev(o), dev(d), 0.0, float(t_max)).cpu().numpy().astype(bool)
    R, rst = LM.lights_mesh_f32(c, trace=scene, occluded=inst)
    tex = c.ref().tex
    quads = np.array([LC.record_kind(r) == "quad" for r in c.lights])
    diff = np.abs(F[:, tex].astype(np.float64) - R[:, tex].astype(np.float64))
    bound = LC.rounding_bound(c)
    sure = LC.all_certain(c)
    same = np.array_equal(bits(F[quads][:, tex]), bits(R[quads][:, tex]))
    print("irt_lights_mesh %-12s against lights_mesh_f32: the quads' bits %s; %d of %d values differ in all; stats %s / %s"
          % (name, "agree" if same else "differ", int((diff > 0).sum()), diff.size, st.tolist(), rst.tolist()))
    # quads: the sample's direction is the same bits on both sides, so the visibility answers are the same questions: every texel, within twice the bound
    assert (diff[quads] <= 2 * bound[quads]).all()
    # spheres: sinf / cosf differ between the two machines: the texels on which every sample is certain, within the bound
    assert (diff[~quads][sure[~quads]] <= bound[~quads][sure[~quads]]).all()
    assert (F[:, np.setdiff1d(np.arange(c.Nt), tex)] == SENTINEL).all()


# ---- 6. monotone and zero --------------------------------------------------------------------------------------------------------------------------------------------

def test_the_objects_only_take_light_and_an_enclosed_light_gives_plus_zero(tx):
    for c in [LM.case(n) for n in ("table", "cube", "twice", "eight", "s24", "inside_box")] + [LM.spec_case(n) for n in ("table", "cube", "twice", "eight")]:
        got, st = run(tx, c)
        plain, st0 = run(tx, c, objects=False)
        rows = c.ref().tex
        assert (got[:, rows] <= plain[:, rows]).all(), c.name
        assert (got[:, rows] < plain[:, rows]).any(), "%s: the objects take nothing" % c.name
        assert st[0] == st0[0] and st[1] < st0[1], c.name
    c = LM.case("enclosed")
    got, st = run(tx, c)
    plain, st0 = run(tx, c, objects=False)
    assert not bits(got[:, c.ref().tex]).any(), "not exactly +0"
    assert st[0] == st0[0] > 0 and st[1] == 0 and (plain[:, c.ref().tex] > 0).any()
    c = LM.case("inside_box")
    got, _ = run(tx, c)
    assert not bits(got[0, c.ref().tex]).any() and (got[1, c.ref().tex] > 0).any()


# ---- 7. purity -------------------------------------------------------------------------------------------------------------------------------------------------------

def test_result_is_a_pure_function_of_the_inputs(tx):
    import ctypes as C
    from texir_code_amd import _lib
    c = LM.case("table")
    sc = scene_of(tx, c.geo)
    base, st = run(tx, c)
    again, st2 = run(tx, c)
    assert np.array_equal(bits(base), bits(again)) and st.tolist() == st2.tolist(), "second run"
    perm = np.random.default_rng(3).permutation(len(c.ids))
    assert np.array_equal(bits(base), bits(run(tx, c, ids=c.ids[perm])[0])), "shuffled list"
    assert np.array_equal(bits(base), bits(run(tx, c, ids=np.concatenate([c.ids, c.ids[:70], [-5, c.Nt, 2 ** 31 - 1]]))[0])), "duplicates and ids outside the atlas"
    cut = torch.full((c.K, c.Nt), SENTINEL, device="cuda")
    for part in (c.ids[:1], c.ids[1:70], c.ids[70:]):
        sc.irt_lights(dev(c.pos), dev(c.nrm), dev(c.shift), torch.from_numpy(c.lights), c.S, texel_ids=dev(part), t_max=c.t_max, out=cut, **objects_of(tx, c))
    assert np.array_equal(bits(base), bits(cut.cpu().numpy())), "cut lists"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run(tx, c)[0]
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(base), bits(on_side)), "side stream"
    # a recorded graph on caller-owned buffers with guard words behind F; the matrices live on the device and are overwritten between replays
    L = _lib.lib()
    pos, nrm, shift, ids, lights = dev(c.pos), dev(c.nrm), dev(c.shift), dev(c.ids), dev(c.lights)
    occ = [occluder_of(tx, n) for n in c.occ]
    handles = (C.c_void_p * len(occ))(*[o.h for o in occ])
    inst = np.array(c.inst, np.int32)
    w2o = dev(c.w2o)
    Kl, Nt, guard = c.K, c.Nt, 64
    out = torch.full((Kl * Nt + guard,), SENTINEL, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                               # the single call on one stream: no parallel branches
            _lib.check(L.texir_irt_lights_mesh(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), ids.numel(), Nt, _lib.ptr(lights), Kl, c.S, c.t_max,
                                               C.cast(handles, C.c_void_p), len(occ), _lib.ptr(inst), _lib.ptr(w2o), c.J, 0, _lib.ptr(out), _lib.ptr(stats),
                                               _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)

    def replay(want, want_st, what):
        out.fill_(SENTINEL)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(want), bits(out[:Kl * Nt].reshape(Kl, Nt).cpu().numpy())), what
        assert stats.cpu().tolist() == want_st.tolist(), what
        assert (out[Kl * Nt:] == SENTINEL).all(), "guard words"
    replay(base, st, "graph replay")
    replay(base, st, "second graph replay")
    moved = MC.to_world_to_object(MC.TABLE_AT(3.0, 2.2, 65.0)[None])
    w2o.copy_(torch.from_numpy(moved))
    fresh, st1 = run(tx, c, w2o=dev(moved))
    assert not np.array_equal(bits(fresh), bits(base))
    replay(fresh, st1, "graph replay after the matrices were overwritten on the device")
    nan = moved.copy()
    nan[0, 5] = np.nan                                                        # a matrix with a non-finite entry never blocks
    w2o.copy_(torch.from_numpy(nan))
    plain, st0 = run(tx, c, objects=False)
    replay(plain, st0, "graph replay with a NaN matrix")


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise_and_empty_calls_write_nothing(tx, monkeypatch):
    import ctypes as C
    from texir_code_amd import _lib
    c, cs = LM.case("s24"), LM.spec_case("table")
    sc = scene_of(tx, c.geo)
    occ = [occluder_of(tx, n) for n in c.occ]
    ids = dev(c.ids)
    out = torch.full((c.K, c.Nt), SENTINEL, device="cuda")
    outs = torch.full((cs.K, cs.P), SENTINEL, device="cuda")
    fl = lambda **kw: sc.irt_lights(dev(c.pos), dev(c.nrm), dev(c.shift), kw.pop("lights", torch.from_numpy(c.lights)), kw.pop("S", c.S), texel_ids=kw.pop("ids", ids),
                                    out=kw.pop("out", out), occluders=kw.pop("occ", occ), instances=kw.pop("inst", c.inst), poses=kw.pop("poses", c.poses), **kw)
    fs = lambda **kw: sc.spec_lights(dev(cs.pos), dev(cs.nrm), dev(cs.rough), dev(cs.shift), dev(cs.cam), torch.from_numpy(cs.lights), kw.pop("S", cs.S),
                                     texel_ids=dev(cs.ids), out=outs, occluders=kw.pop("occ", occ), instances=kw.pop("inst", c.inst), poses=kw.pop("poses", c.poses), **kw)
    for call, fn in ((fl, "texir_irt_lights_mesh"), (fs, "texir_spec_lights_mesh")):
        with pytest.raises(_lib.TexirError, match=fn + ": Q must be in 0..8, got 9"):
            call(occ=[occ[0]] * 9)
        with pytest.raises(_lib.TexirError, match=fn + ": J must be in 0..8, got 9"):
            call(inst=[0] * 9, poses=np.tile(MC.pose()[None], (9, 1, 1)))
        with pytest.raises(_lib.TexirError, match=fn + r": inst_obj\[1\] = 2 names no occluder \(Q = 2\)"):
            call(inst=[0, 2])
        with pytest.raises(_lib.TexirError, match=fn + r": inst_obj\[0\] = -1 names no occluder"):
            call(inst=[-1, 1])
        with pytest.raises(_lib.TexirError, match=fn + ": S must be in 1..65536, got 0"):
            call(S=0)
        with pytest.raises(_lib.TexirError, match=fn + ": t_max must be finite"):
            call(t_max=float("inf"))
        with pytest.raises(ValueError, match="pose 1 is singular"):
            call(poses=np.stack([c.poses[0], np.zeros((3, 4))]))
        with pytest.raises(ValueError, match="2 instances, 1 poses"):
            call(poses=c.poses[:1])
        with pytest.raises(ValueError, match="device poses must be"):
            call(poses=torch.zeros((2, 3, 4), device="cuda"))
        with pytest.raises(ValueError, match="occluders must be Scene handles"):
            call(occ=[occ[0], None])
        with pytest.raises(ValueError, match="query must be"):
            call(query="nearest")
    with pytest.raises(_lib.TexirError, match="texir_irt_lights_mesh: K must be in 0..8, got 9"):
        fl(lights=torch.zeros((9, 16)), out=torch.zeros((9, c.Nt), device="cuda"))
    with pytest.raises(_lib.TexirError, match="clamp_eps must be finite and > 0"):
        fs(clamp_eps=0.0)
    # empty calls: an empty list, no lights
    assert fl(ids=ids[:0]) is out
    none = torch.full((0, c.Nt), SENTINEL, device="cuda")
    assert fl(lights=torch.zeros((0, 16)), out=none) is none
    L = _lib.lib()
    pos, nrm, shift, lights, w2o, inst = dev(c.pos), dev(c.nrm), dev(c.shift), dev(c.lights), dev(c.w2o), np.array(c.inst, np.int32)

    def raw(n_ids, s=sc, handles=occ, mats=w2o):
        hs = (C.c_void_p * len(handles))(*[o.h for o in handles])
        return L.texir_irt_lights_mesh(s.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, c.Nt, _lib.ptr(lights), c.K, c.S, c.t_max,
                                       C.cast(hs, C.c_void_p), 2, _lib.ptr(inst), _lib.ptr(mats), 2, 0, _lib.ptr(out), None, _lib.stream_ptr())
    _lib.check(raw(0))                                                        # a non-null empty list is a no-op
    with pytest.raises(_lib.TexirError, match="inst_world_to_obj is null"):
        _lib.check(raw(65, mats=None))
    monkeypatch.setenv("TEXIR_BVH_WIDTH", "2")
    binary = tx.Scene(c.geo.verts, c.geo.tris, c.geo.tri_uvs, c.geo.hdr)
    g = MC.occluder("ico")
    binary_occ = tx.Scene.occluder(g.verts, g.tris)
    monkeypatch.delenv("TEXIR_BVH_WIDTH")
    with pytest.raises(_lib.TexirError, match="texir_irt_lights_mesh: the scene has no 4-wide tree"):
        _lib.check(raw(65, binary))
    with pytest.raises(_lib.TexirError, match=r"texir_irt_lights_mesh: occluders\[1\] has no 4-wide tree"):
        _lib.check(raw(65, sc, [occ[0], binary_occ]))
    if torch.cuda.device_count() > 1:
        other = tx.Scene.occluder(g.verts, g.tris, device=1)
        with pytest.raises(_lib.TexirError, match=r"occluders\[1\] lives on device 1, the scene on device 0"):
            _lib.check(raw(65, sc, [occ[0], other]))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (outs == SENTINEL).all()


# ---- 9. host and device poses ----------------------------------------------------------------------------------------------------------------------------------------

def test_host_poses_and_device_matrices_give_the_same_bits(tx):
    for c in (LM.case("cube"), LM.case("s24"), LM.spec_case("cube")):
        onw, st = run(tx, c)
        host, st_h = run(tx, c, objects=False, occluders=[occluder_of(tx, n) for n in c.occ], instances=c.inst, poses=c.poses)
        assert np.array_equal(bits(onw), bits(host)) and st.tolist() == st_h.tolist(), c.name
        four = np.concatenate([c.poses, np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (c.J, 1, 1))], 1)
        assert np.array_equal(bits(onw), bits(run(tx, c, objects=False, occluders=[occluder_of(tx, n) for n in c.occ], instances=c.inst, poses=torch.from_numpy(four))[0]))


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------------------------------------------

def test_stage_writes_the_object_light_files_and_light_irt_takes_them(tmp_path, capsys):
    from texir_code_amd import datasets as D, io_formats as IO, tools
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
    a, b = [0.15 * ext[0], 0, 0], [0, 0, 0.15 * ext[2]]
    lights = {"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                         {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.05 * float(ext.min())}]}
    ljs = str(tmp_path / "lights.json")
    with open(ljs, "w") as f:
        json.dump(lights, f)
    g = MC.occluder("table")
    obj = str(tmp_path / "table.obj")
    with open(obj, "w") as f:
        f.write("".join("v %r %r %r\n" % tuple(float(x) for x in v) for v in g.verts) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in g.tris))
    s = 0.3 * float(ext.min())
    objects = [{"obj": obj, "pose": {"translate": [float(ctr[0]), float(lo[1]), float(ctr[2])], "rotate_deg": [0, 20, 0], "scale": s}}]
    keys = ['irt_lights = "%s"' % ljs, "irt_light_samples = 16", "irt_objects = " + json.dumps(objects), "irt_object_samples = 16"]
    d0, plain = stage("plain", keys)                                              # the parent behaviour: lights and objects, the new key absent
    d1, off = stage("off", keys + ["irt_light_objects = false"])
    d2, on = stage("on", keys + ["irt_light_objects = true"])
    assert sorted(off) == sorted(plain) and all(off[f] == plain[f] for f in plain), "false: the listing and every file byte for byte"
    assert sorted(set(on) - set(plain)) == ["0_irr_texture_light0_objects.hdr", "0_irr_texture_light1_objects.hdr"]
    assert all(on[f] == plain[f] for f in plain), "every other file is byte-identical with and without the key"
    rd = lambda name: IO.read_hdr(os.path.join(d2, name)).astype(np.float64)
    for k in (0, 1):
        F, Fo = rd("0_irr_texture_light%d.hdr" % k), rd("0_irr_texture_light%d_objects.hdr" % k)
        # an RGBE pixel keeps 8 bits below its largest channel's power of two: the files are rounded separately
        assert Fo.shape == F.shape and (Fo <= F + 2.0 ** -7 * F.max(-1)[..., None] + 1e-6).all()
        darker = (Fo[..., 0] < 0.5 * F[..., 0]) & (F[..., 0] > 0)
        same = (Fo == F).all(-1) & (F[..., 0] > 0)
        with capsys.disabled():
            print("stage: light %d: %d texels lose more than half of their factor to the table, %d keep it" % (k, int(darker.sum()), int(same.sum())))
        assert darker.sum() > 0 and same.sum() > darker.sum(), "the table must shadow some texels and leave most as they are"
    with pytest.raises(ValueError, match="train.irt_light_objects = true needs train.irt_lights .* and train.irt_objects"):
        stage("lonely", keys[:2] + ["irt_light_objects = true"])
    assert tools.main(["light-irt", d2, "--objects", "--light", "0", "--colour", "20,18,15", "--light", "1", "--colour", "5,5,9"]) == 0
    got = rd("0_irr_texture_lit.hdr")
    want = rd("0_irr_texture.hdr") + rd("0_irr_texture_light0_objects.hdr") * np.array([20.0, 18.0, 15.0]) + rd("0_irr_texture_light1_objects.hdr") * np.array([5.0, 5.0, 9.0])
    assert (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    capsys.readouterr()
    assert tools.main(["light-irt", d0, "--objects", "--light", "0", "--colour", "1,1,1"]) == 1      # no object files there
    assert "train.irt_light_objects" in capsys.readouterr().out


# ---- 11. the evaluation model ----------------------------------------------------------------------------------------------------------------------------------------

def test_evaluation_model_with_test_objects_is_render_plus_add_view_of_the_shadowed_factors(tx, tmp_path):
    from texir_code_amd import irtlight
    from texir_code_amd.tester import lit_model as LIT, test_model as TM
    geo, pos, nrm, shift, v, lo, hi = LC.room_inputs()
    pick = v[5::len(v) // 384][:384]                                       # a 6 x 8 x 8 G-buffer of points the room really has
    shape = (6, 8, 8)
    rng = np.random.default_rng(17)
    normal, points = dev(nrm[pick].reshape(shape + (3,))), dev(pos[pick].reshape(shape + (3,)))
    albedo, irr = dev(rng.random(shape + (3,), dtype=np.float32)), dev(rng.random(shape + (3,), dtype=np.float32))
    rough = dev(SL.room_rough(384, 3).reshape(shape + (1,)))
    cam = dev(SL.room_cam())
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.3 * ext[0], 0, 0], [0, 0, 0.3 * ext[2]]
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                                         {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.1 * float(ext.min())}]}))
    g = MC.occluder("table")
    obj = tmp_path / "table.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in q) for q in g.verts) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in g.tris))
    spec = [{"obj": str(obj), "pose": {"translate": [float(ctr[0]), float(lo[1]), float(ctr[2])], "rotate_deg": [0, 20, 0], "scale": 2.0}}]
    m = LIT.MaterialModel.__new__(LIT.MaterialModel)
    torch.nn.Module.__init__(m)
    m.scene = scene_of(tx, geo)
    m.device, m.sample_l, m.sample_type, m.relighting = m.scene.device, [16, 16], ["uniform", "importance"], False
    torch.manual_seed(5)
    plain = m.render(normal, albedo, rough, points, cam, irr)
    m.test_lights, m.light_samples = LIT.load_test_lights(str(js), m.device), 32
    m.test_objects = LIT.load_test_objects("none", m.test_lights, m.device)
    assert m.test_objects is None
    torch.manual_seed(5)
    lit = m.render(normal, albedo, rough, points, cam, irr)
    torch.manual_seed(5)
    shift_s = torch.rand(384, 1, 2).reshape(384, 2).cuda()                 # the pixels' own specular shift
    records, colours = m.test_lights
    flat = (points.reshape(-1, 3), normal.reshape(-1, 3))
    F0 = m.scene.irt_lights(*flat, shift_s, records, 32)
    R0 = m.scene.spec_lights(*flat, rough.reshape(-1), shift_s, cam, records, 32, clamp_eps=TM.TINY_NUMBER)
    want0 = irtlight.add_view(plain["rgb"].reshape(-1, 3), albedo.reshape(-1, 3), F0, R0, colours).reshape(shape + (3,))
    assert torch.equal(lit["rgb"], want0), "test.objects = none: render() is what it was"
    m.test_objects = LIT.load_test_objects(spec, m.test_lights, m.device)
    torch.manual_seed(5)
    state = None
    shadowed = m.render(normal, albedo, rough, points, cam, irr)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    m.test_objects = None
    m.render(normal, albedo, rough, points, cam, irr)
    assert torch.equal(torch.get_rng_state(), state), "the objects drew from the CPU generator"
    kw = LIT.load_test_objects(spec, (records, colours), m.device)
    F = m.scene.irt_lights(*flat, shift_s, records, 32, **kw)
    R = m.scene.spec_lights(*flat, rough.reshape(-1), shift_s, cam, records, 32, clamp_eps=TM.TINY_NUMBER, **kw)
    want = irtlight.add_view(plain["rgb"].reshape(-1, 3), albedo.reshape(-1, 3), F, R, colours).reshape(shape + (3,))
    assert torch.equal(shadowed["rgb"], want) and not torch.equal(shadowed["rgb"], lit["rgb"])
    assert (F <= F0).all() and (F < F0).any() and (R <= R0).all()
    for k in ("albedo", "normal", "position"):
        assert torch.equal(shadowed[k], plain[k])
