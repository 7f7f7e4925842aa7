"""GPU: the atlas bake (texir_atlas_bake / texir_atlas_gather, csrc/texbake.hip; atlas.bake_atlas; `tools bake-atlas`) against the float64 reference of its
rule (atlas_bake_cases.py states the rule, the margins and the cases; test_atlas_bake_ref_cpu.py shows the checker rejects seven mutants and asserts the caps).

Every listed texel of every case: (view, row, col) is an admissible outcome and rgb is that panorama pixel bit for bit; unlisted texels keep a sentinel.

Run on an MI355X: 26 passed.  On every case the device's `stats` counters (pairs facing, traced, visible, texels assigned) equal those of the float32
restatement of the header's arithmetic (atlas_bake_cases.bake_f32), e.g. room96: 47 501 / 28 723 / 10 208 / 4 973; the device convention pin agrees on 99.67 %
of 98 304 covered face pixels, worst offset one pixel.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import atlas_bake_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = (-7, 5, 0.25)


@pytest.fixture(scope="module")
def scenes(tx):
    cache = {}

    def get(geo):
        if geo.name not in cache:
            cache[geo.name] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr, device=0)
        return cache[geo.name]
    return get


def _run(sc, case, ids="case", stats=False, panos=None):
    from texir_code_amd import atlas
    ids = case.ids if isinstance(ids, str) else ids
    out = (torch.full((case.Nt,), SENTINEL[0], device="cuda", dtype=torch.int32), torch.full((case.Nt, 2), SENTINEL[1], device="cuda", dtype=torch.int32),
           torch.full((case.Nt, 3), SENTINEL[2], device="cuda", dtype=torch.float32))
    res = atlas.bake_atlas(sc, torch.from_numpy(case.pos), torch.from_numpy(case.nrm), torch.from_numpy(case.Wm), torch.from_numpy(case.cam),
                           torch.from_numpy(case.panos() if panos is None else panos), None if case.valid is None else torch.from_numpy(case.valid),
                           case.cos_min, None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, np.int32)), out=out, stats=stats)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _bits(a):
    return [x.view(np.uint32) if x.dtype == np.float32 else x for x in a]


def test_entry_points_exist():
    from texir_code_amd import _lib, atlas
    L = _lib.lib()
    assert hasattr(L, "texir_atlas_bake") and hasattr(L, "texir_atlas_gather")
    assert callable(atlas.bake_atlas) and callable(atlas.gather_atlas)


@pytest.mark.parametrize("name", C.ALL)
def test_every_texel_admissible(scenes, name):
    case = C.case(name)
    ref = case.ref()
    assert ref.caps() <= C.CAP_MULTI                                      # from the reference alone, before the device is asked
    view, pix, rgb, st = _run(scenes(case.geo), case, stats=True)
    fails = C.check(case, view, pix, rgb, sentinel=SENTINEL)
    print(name, ref.stats(), "device stats", st.tolist())
    assert not fails, (len(fails), fails[:5])
    # the counters, where the outputs determine them
    assigned = int((view[ref.tex] >= 0).sum())
    assert st[3] == assigned and st[2] >= assigned and st[0] >= st[1] >= st[2]
    if name == "closed_box":
        assert (view == -1).all() and not pix.any() and not rgb.any()
    if name == "tie":
        assert (view == 0).all()


@pytest.mark.parametrize("name", ["room64", "list65", "room64_mask"])
def test_list_order_and_repetition_do_not_change_a_bit(scenes, name):
    case = C.case(name)
    sc = scenes(case.geo)
    a, b = _run(sc, case), _run(sc, case)
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))
    perm = np.random.default_rng(9).permutation(case.listed()).astype(np.int32)
    c = _run(sc, case, ids=perm)
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(c)))


def test_null_list_equals_the_full_list(scenes):
    case = C.case("null200")
    sc = scenes(case.geo)
    a = _run(sc, case)
    b = _run(sc, case, ids=np.arange(case.Nt, dtype=np.int32))
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))
    assert (a[0] != SENTINEL[0]).all()


def test_rgb_is_copied_bit_for_bit(scenes):
    """arbitrary bit patterns in the panoramas (a NaN payload, a denormal, -0.0 among them) arrive unchanged"""
    case = C.case("list200")
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2 ** 32, (case.K, case.h, case.w, 3), dtype=np.uint64).astype(np.uint32)
    bits[0, 0, 0] = (0x7FC12345, 0x00000001, 0x80000000)
    panos = bits.view(np.float32)
    view, pix, rgb = _run(scenes(case.geo), case, panos=panos)
    got = view >= 0
    assert got.sum() > 50
    assert np.array_equal(rgb.view(np.uint32)[got], bits[view[got], pix[got, 0], pix[got, 1]])


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_gather_equals_torch_indexing(scenes, Cn):
    from texir_code_amd import atlas
    case = C.case("room64_rot")
    view, pix, _ = _run(scenes(case.geo), case)
    view[view == SENTINEL[0]] = -1
    pix[view < 0] = 0
    rng = np.random.default_rng(Cn)
    imgs = torch.from_numpy(rng.uniform(-5, 5, (case.K, case.h, case.w, Cn)).astype(np.float32)).cuda()
    v, p = torch.from_numpy(view).cuda(), torch.from_numpy(pix).cuda()
    out = atlas.gather_atlas(v, p, imgs)
    want = imgs[v.clamp(min=0).long(), p[:, 0].long(), p[:, 1].long()] * (v >= 0)[:, None]
    assert out.shape == (case.Nt, Cn) and torch.equal(out, want)
    # a listed subset leaves the others alone
    ids = torch.arange(0, case.Nt, 3, device="cuda", dtype=torch.int32)
    part = atlas.gather_atlas(v, p, imgs, texel_ids=ids, out=torch.full((case.Nt, Cn), 9.0, device="cuda"))
    keep = torch.ones(case.Nt, dtype=torch.bool, device="cuda")
    keep[ids.long()] = False
    assert torch.equal(part[ids.long()], want[ids.long()]) and (part[keep] == 9.0).all()


def test_argument_errors(scenes):
    from texir_code_amd import _lib, atlas
    case = C.case("list64")
    sc = scenes(case.geo)
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pos, nrm, Wm, cam, panos = t(case.pos), t(case.nrm), t(case.Wm), t(case.cam), t(case.panos())
    view, pix, rgb = torch.zeros(case.Nt, dtype=torch.int32, device="cuda"), torch.zeros(case.Nt, 2, dtype=torch.int32, device="cuda"), torch.zeros(case.Nt, 3, device="cuda")
    P = _lib.ptr

    def bake(K=case.K, h=case.h, w=case.w, view_=view, panos_=panos, scene=sc.h):
        return L.texir_atlas_bake(scene, P(pos), P(nrm), None, 0, case.Nt, P(Wm), P(cam), P(panos_), None, K, h, w, 0.1, P(view_), P(pix), P(rgb), None, _lib.stream_ptr())
    for kw, word in (({"K": 0}, "K must be"), ({"h": 0}, "h and w"), ({"w": -3}, "h and w"), ({"view_": None}, "null output"), ({"panos_": None}, "null argument"),
                     ({"scene": None}, "null argument")):
        with pytest.raises(_lib.TexirError, match=word):
            _lib.check(bake(**kw))
    with pytest.raises(_lib.TexirError, match="C must be"):
        _lib.check(L.texir_atlas_gather(P(view), P(pix), None, 0, case.Nt, P(panos), case.K, case.h, case.w, 5, P(rgb), _lib.stream_ptr()))
    with pytest.raises(_lib.TexirError, match="null output"):
        _lib.check(L.texir_atlas_gather(P(view), P(pix), None, 0, case.Nt, P(panos), case.K, case.h, case.w, 3, None, _lib.stream_ptr()))
    with pytest.raises(ValueError):
        atlas.bake_atlas(sc, pos, nrm, Wm[:2], cam, panos)
    torch.cuda.synchronize()


def test_graph_capture_and_replay(scenes):
    """caller-owned buffers, no allocation, no synchronisation: the call records into a graph and the replay writes the eager run's bits"""
    from texir_code_amd import _lib
    case = C.case("room64_mask")
    sc = scenes(case.geo)
    want = _run(sc, case, stats=True)
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pos, nrm, Wm, cam, panos, valid, ids = t(case.pos), t(case.nrm), t(case.Wm), t(case.cam), t(case.panos()), t(case.valid), t(case.ids)
    view = torch.zeros(case.Nt, dtype=torch.int32, device="cuda")
    pix = torch.zeros(case.Nt, 2, dtype=torch.int32, device="cuda")
    rgb = torch.zeros(case.Nt, 3, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_atlas_bake(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(ids), ids.numel(), case.Nt, _lib.ptr(Wm), _lib.ptr(cam), _lib.ptr(panos),
                                          _lib.ptr(valid), case.K, case.h, case.w, case.cos_min, _lib.ptr(view), _lib.ptr(pix), _lib.ptr(rgb), _lib.ptr(st),
                                          _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        view.fill_(SENTINEL[0]); pix.fill_(SENTINEL[1]); rgb.fill_(SENTINEL[2]); st.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = [view.cpu().numpy(), pix.cpu().numpy(), rgb.cpu().numpy(), st.cpu().numpy()]
        assert all(np.array_equal(x, y) for x, y in zip(_bits(got), _bits(want)))


def test_convention_pin_on_the_device(tx):
    """pano_pixel(camera_matrices(E)) at MaterialModel._gbuffer's positions names the panorama pixel Pano2Cube shows at the same face pixel: >= 99 % of the
    covered face pixels exactly, the rest one pixel off.  Sizes: the G-buffer samples pixel centres, Pano2Cube corner-aligned positions, up to half a face
    pixel apart; at c = 128 against 5 x 12 the two sample positions alone agree on 99.65 % (test_atlas_bake_ref_cpu.test_pixel_centres_against_the_grid)."""
    from texir_code_amd import atlas, cameras, conf as CF, synth
    from texir_code_amd.models import MaterialModel
    from texir_code_amd.pano2cube import Pano2Cube
    c, h, w = 128, 5, 12
    s = synth.make_scene(2000, tex_res=64)
    sc = tx.Scene(s["verts"], s["tris"], s["tri_uvs"], s["hdr"], device=0)
    conf = CF.parse_string("train{ pano_img_res = [%d,%d]\n sample_light = [64,16]\n hdr_exposure = 0 }\nmodels{ render{ sample_type = [uniform, importance] } }" % (2 * c, 4 * c))
    model = MaterialModel.from_arrays(sc, s["hdr"], np.zeros((8, 8, 3), np.float32), conf, albedo_res=8, roughness_res=8)
    E = cameras.grid_cameras(2)[1].astype(np.float64)
    E[:3, :3] = C.random_rotation(np.random.default_rng(12))
    mvp, _ = cameras.cube_mvps(E.astype(np.float32))
    gb = model._gbuffer(mvp, "pin")
    pos, mask = gb["position"].cpu().double(), gb["mask"].cpu().reshape(6, c, c) > 0
    Wm, _ = atlas.camera_matrices(E[None])
    row, col = atlas.pano_pixel(Wm[0], pos, h, w)
    pano = torch.zeros(1, 2, h, w)
    r, cc = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pano[0, 0], pano[0, 1] = r, cc
    cube = Pano2Cube(1, w, h, c, 2).Tocube(pano, "nearest")[0].reshape(6, 2, c, c)
    dr = (row - cube[:, 0].long()).abs()
    dc = (col - cube[:, 1].long()).abs()
    dc = torch.minimum(dc, w - dc)
    assert mask.float().mean() > 0.9
    share = float(((dr == 0) & (dc == 0))[mask].float().mean())
    print("device convention pin: %.4f of %d covered face pixels agree, worst offset %d" % (share, int(mask.sum()), int(torch.maximum(dr, dc)[mask].max())))
    assert share >= 0.99 and int(torch.maximum(dr, dc)[mask].max()) <= 1


def test_end_to_end_files_and_irt_stage(tx, tmp_path):
    """96^2 with 3 x 3 views of 50 x 100: write_synthetic_dataset + trace_panoramas written as ccm.hdr -> `bake-atlas` -> the files equal bake_atlas' arrays (the
    .hdr bit for bit: the inputs are RGBE-born; the codes exactly) -> --trainstage IrrT with train.texel_gbuffer = raster on the baked directory gives a finite,
    non-zero irradiance, and the baked directory's scene reports the 4-byte texel layout"""
    from texir_code_amd import atlas, conf as CF, datasets as D, dist_util, gbuffer as GB, io_formats as IO, models, tools
    from texir_code_amd.trainer import exp_runner as ER
    root = str(tmp_path / "data")
    s = D.write_synthetic_dataset(root, T=2000, texel_res=96, tex_res=64, n_side=3)
    mesh_dir = os.path.join(root, "vrproc", "hdr_texture")
    E = atlas.read_extrinsics(root)
    ids = [l.strip() for l in open(os.path.join(root, "info", "aligned.txt")) if l.strip()]
    assert E.shape[0] == len(ids) == 9
    lit = tx.Scene(s["verts"], s["tris"], s["tri_uvs"], s["hdr"], device=0)
    traced = atlas.trace_panoramas(lit, E, 50, 100).cpu().numpy()
    assert np.isfinite(traced).all() and (traced.sum(-1) > 0).mean() > 0.9
    for k, i in enumerate(ids):
        os.makedirs(os.path.join(root, "hdr", i))
        IO.write_hdr(os.path.join(root, "hdr", i, "ccm.hdr"), traced[k])
    root2 = str(tmp_path / "baked")
    out_dir = os.path.join(root2, "vrproc", "hdr_texture")
    assert tools.main(["bake-atlas", root, "96", "--out", out_dir]) == 0
    assert tools.main(["bake-atlas", root, "96", "--out", out_dir]) == 1          # refuses to overwrite
    hdr = IO.read_hdr(os.path.join(out_dir, "hdr_texture.hdr"))
    idx = IO.read_index_texture(os.path.join(out_dir, "0.png"))
    assert hdr.shape == (96, 96, 3) and idx.shape == (96, 96, 3) and idx.dtype == np.uint16
    # the same bake in this process, from the files the command read
    IO._OBJ_CACHE.clear()
    obj = IO.load_obj(os.path.join(mesh_dir, "out1.obj"))
    sc = tx.Scene(obj["vertices"], obj["indices"], IO.triangle_uvs_open3d(obj), np.zeros((2, 2, 3), np.float32), device=0)
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(sc, 96, 96, want_ids=True)
    order = dist_util.morton_order(torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32), 96)
    panos = np.stack([IO.read_hdr(os.path.join(root, "hdr", i, "ccm.hdr")) for i in ids], 0)
    Wm, cam = atlas.camera_matrices(E)
    view, pix, rgb = atlas.bake_atlas(sc, pos, nrm, Wm, cam, panos, texel_ids=order)
    torch.cuda.synchronize()
    view, pix, rgb = view.cpu().numpy(), pix.cpu().numpy(), rgb.cpu().numpy()
    got = view >= 0
    assert got.sum() > 0.5 * order.numel()
    assert np.array_equal(rgb.view(np.uint32)[got], panos[view[got], pix[got, 0], pix[got, 1]].view(np.uint32))
    assert np.array_equal(hdr.reshape(-1, 3).view(np.uint32), rgb.view(np.uint32))           # RGBE-born pixels survive the RGBE file bit for bit
    assert np.array_equal(idx.reshape(-1, 3), atlas.index_codes(view, pix, 50, 100))
    v2, p2 = atlas.decode_codes(idx.reshape(-1, 3), 50, 100)
    assert np.array_equal(v2, view) and np.array_equal(p2, pix)
    # the baked directory as a dataset of its own: mesh + info beside the two files
    shutil.copy(os.path.join(mesh_dir, "out1.obj"), os.path.join(out_dir, "out1.obj"))
    shutil.copytree(os.path.join(root, "info"), os.path.join(root2, "info"))
    conf_path = str(tmp_path / "irt.conf")
    D.write_conf(conf_path, root2, cube_res=16, spp=(64, 16), model="irt")
    txt = open(conf_path).read()
    open(conf_path, "w").write(txt.replace("irt_res = native", "irt_res = native\n    texel_gbuffer = raster"))
    IO._OBJ_CACHE.clear()
    ER.main(["--conf", conf_path, "--trainstage", "IrrT", "--gpu", "0"])
    irr = IO.read_hdr(os.path.join(out_dir, "0_irr_texture.hdr"))
    assert irr.shape == (96, 96, 3) and np.isfinite(irr).all() and (irr.sum(-1) > 0).sum() > 0.5 * order.numel()
    scene, _, _ = models._load_scene(CF.ConfigFactory.parse_file(conf_path), 0)
    assert scene.texture_layout() >= 3, scene.texture_layout()
