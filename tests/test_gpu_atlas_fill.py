"""GPU: the atlas fill (texir_atlas_fill, csrc/texfill.hip; atlas.fill_atlas, atlas.dilate_gutters; `tools bake-atlas --fill`) against the float32 restatement
of its rule (atlas_fill_cases.fill_f32; test_atlas_fill_ref_cpu.py shows that restatement admissible under the float64 reference and the checker's teeth).

Only IEEE subtractions, products, sums and comparisons occur, so the device must give fill_f32's bits: src and dist2 of every listed hole of every case, the
sentinel on every unlisted texel, the two counters; and the same bits whatever the order of the lists, the cell size, the box, the stream, eager or replayed
from a graph.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import atlas_fill_cases as C

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(case, sources=None, holes=None, cell=0.0, bounds=None, stats=True):
    from texir_code_amd import atlas
    out = (torch.full((case.Nt,), C.SENTINEL[0], device="cuda", dtype=torch.int32), torch.full((case.Nt,), C.SENTINEL[1], device="cuda", dtype=torch.float32))
    res = atlas.fill_atlas(_dev(case.pos), _dev(case.nrm), _dev(case.sources if sources is None else sources), _dev(case.holes if holes is None else holes),
                           case.cos_fill, case.max_dist, bounds=case.bounds if bounds is None else bounds, out=out, stats=stats, dist2=True, cell=cell)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_entry_points_exist():
    from texir_code_amd import _lib, atlas
    L = _lib.lib()
    assert hasattr(L, "texir_atlas_fill") and hasattr(L, "texir_atlas_fill_workspace_bytes")
    assert callable(atlas.fill_atlas) and callable(atlas.dilate_gutters)


@pytest.mark.parametrize("name", C.ALL)
def test_bits_of_the_float32_restatement(name):
    case = C.case(name)
    want = case.f32()
    src, dist2, st = _run(case)
    H = case.valid_holes()
    diff = np.nonzero(src != want[0])[0]
    print(name, "holes", len(H), "sources", len(case.valid_sources()), "filled", int((want[0][H] >= 0).sum()), "device stats", st.tolist(), "differing", len(diff))
    assert not len(diff), [(int(t), int(src[t]), int(want[0][t])) for t in diff[:5]]
    assert np.array_equal(dist2.view(np.uint32), want[1].view(np.uint32))     # unlisted texels keep the sentinel: want holds it there
    assert st.tolist() == want[2].tolist()


@pytest.mark.parametrize("name", ["room64_bake", "room96_balls", "dup_oor", "lattice_tie", "list_h257_s3000"])
def test_variations_do_not_change_a_bit(name):
    from texir_code_amd import atlas
    case = C.case(name)
    want = case.f32()
    rng = np.random.default_rng(9)
    assert _same(_run(case, sources=rng.permutation(case.sources), holes=rng.permutation(case.holes)), want)            # both lists shuffled
    cell = atlas.fill_cell(case.bounds, len(case.sources))
    assert cell > 0
    for f in (0.25, 4.0):
        assert _same(_run(case, cell=f * cell), want), f
    b = case.bounds.astype(np.float64)
    mid, half = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
    for f in (0.5, 0.0):                                                   # the box shrunk to half its size, and to a point
        assert _same(_run(case, bounds=np.concatenate([mid - f * half, mid + f * half])), want), f
    assert _same(_run(case), want)                                         # a second run
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(case)
    torch.cuda.current_stream().wait_stream(side)
    assert _same(got, want)


def test_graph_capture_and_guard_words():
    """caller-owned buffers, no allocation, no synchronisation: the call records into a graph and each replay writes fill_f32's bits; the words after
    workspace_bytes stay intact"""
    from texir_code_amd import _lib
    case = C.case("room96_balls")
    want = case.f32()
    L, P = _lib.lib(), _lib.ptr
    pos, nrm, sid, hid = _dev(case.pos), _dev(case.nrm), _dev(case.sources), _dev(case.holes)
    src = torch.zeros(case.Nt, dtype=torch.int32, device="cuda")
    d2 = torch.zeros(case.Nt, dtype=torch.float32, device="cuda")
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    nb = int(L.texir_atlas_fill_workspace_bytes(sid.numel(), hid.numel()))
    assert nb > 0 and nb % 4 == 0
    GUARD = 0x5A5A5A5A
    ws = torch.full((nb // 4 + 1024,), GUARD, dtype=torch.int32, device="cuda")
    bounds = np.ascontiguousarray(case.bounds, np.float32)

    def call():
        _lib.check(L.texir_atlas_fill(P(pos), P(nrm), case.Nt, P(sid), sid.numel(), P(hid), hid.numel(), P(bounds), case.cos_fill, case.max_dist, 0.0, P(src), P(d2),
                                      P(st), P(ws), _lib.stream_ptr()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        src.fill_(C.SENTINEL[0]); d2.fill_(C.SENTINEL[1]); st.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same([src.cpu().numpy(), d2.cpu().numpy()], want) and st.cpu().tolist() == want[2].tolist()
        assert (ws[nb // 4:] == GUARD).all()
    # the smallest cells the workspace admits (a tiny cell is doubled until the grid fits): still inside
    _lib.check(L.texir_atlas_fill(P(pos), P(nrm), case.Nt, P(sid), sid.numel(), P(hid), hid.numel(), P(bounds), case.cos_fill, case.max_dist, 1e-6, P(src), P(d2),
                                  None, P(ws), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert (ws[nb // 4:] == GUARD).all() and _same([src.cpu().numpy(), d2.cpu().numpy()], want)


def test_argument_errors():
    from texir_code_amd import _lib, atlas
    case = C.case("list_h64_s64")
    L, P = _lib.lib(), _lib.ptr
    pos, nrm, sid, hid = _dev(case.pos), _dev(case.nrm), _dev(case.sources), _dev(case.holes)
    src = torch.zeros(case.Nt, dtype=torch.int32, device="cuda")
    ws = torch.zeros(int(L.texir_atlas_fill_workspace_bytes(64, 64)), dtype=torch.uint8, device="cuda")
    ok = np.ascontiguousarray(case.bounds, np.float32)

    def call(bounds=ok, cos=0.5, dist=0.5, cell=0.0, src_=src, ws_=ws):
        return L.texir_atlas_fill(P(pos), P(nrm), case.Nt, P(sid), 64, P(hid), 64, P(bounds), cos, dist, cell, P(src_), None, None, P(ws_), _lib.stream_ptr())
    for kw, word in (({"cos": 1.5}, "cos_fill"), ({"cos": -0.1}, "cos_fill"), ({"dist": 0.0}, "max_dist"), ({"dist": float("nan")}, "max_dist"),
                     ({"cell": -1.0}, "cell"), ({"src_": None}, "null argument"), ({"ws_": None}, "null argument"),
                     ({"bounds": np.array([0, 0, 0, 1, np.inf, 1], np.float32)}, "bounds"), ({"bounds": np.array([0, 0, 0, 1, -1, 1], np.float32)}, "bounds")):
        with pytest.raises(_lib.TexirError, match=word):
            _lib.check(call(**kw))
    with pytest.raises(ValueError):
        atlas.fill_atlas(pos, nrm, sid, hid, cos_fill=2.0)
    # bounds=None takes the listed positions' own box
    got = atlas.fill_atlas(pos, nrm, sid, hid, case.cos_fill, case.max_dist)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy()[case.valid_holes()], case.f32()[0][case.valid_holes()])


def test_dilate_gutters_on_the_device():
    from texir_code_amd import atlas
    rng = np.random.default_rng(5)
    H, W = 37, 50
    cov = np.zeros((H, W), bool)
    cov[3:15, 4:20] = cov[20:33, 10:44] = cov[5:9, 30:47] = True
    img = rng.uniform(0.1, 4.0, (H, W, 3)).astype(np.float32)
    img[~cov] = 0
    img[5:8, 6:9] = 0                                                      # covered and black on purpose
    out = atlas.dilate_gutters(_dev(img), _dev(cov)).cpu().numpy()
    assert np.array_equal(out[cov].view(np.uint32), img[cov].view(np.uint32))
    rr, cc = np.nonzero(cov)
    for r, c_ in zip(*np.nonzero(~cov)):
        d2 = (rr - r) ** 2 + (cc - c_) ** 2
        near = d2 == d2.min()
        assert any(np.array_equal(out[r, c_], img[a, b]) for a, b in zip(rr[near], cc[near])), (r, c_)


@pytest.fixture(scope="module")
def baked(tx, tmp_path_factory):
    """the synthetic dataset directory at 64^2 with 2 x 2 views of 32 x 64, baked without and with --fill"""
    from texir_code_amd import atlas, datasets as D, io_formats as IO, tools
    tmp = tmp_path_factory.mktemp("fill")
    root = str(tmp / "data")
    s = D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
    E = atlas.read_extrinsics(root)
    ids = [l.strip() for l in open(os.path.join(root, "info", "aligned.txt")) if l.strip()]
    lit = tx.Scene(s["verts"], s["tris"], s["tri_uvs"], s["hdr"], device=0)
    traced = atlas.trace_panoramas(lit, E, 32, 64).cpu().numpy()
    for k, i in enumerate(ids):
        os.makedirs(os.path.join(root, "hdr", i))
        IO.write_hdr(os.path.join(root, "hdr", i, "ccm.hdr"), traced[k])
    dirs = {}
    for key, extra in (("plain", []), ("fill", ["--fill"])):
        dirs[key] = os.path.join(str(tmp / key), "vrproc", "hdr_texture")
        assert tools.main(["bake-atlas", root, "64", "--out", dirs[key]] + extra) == 0
    return {"root": root, "tmp": tmp, "ids": ids, "E": E, "dirs": dirs}


def test_without_fill_the_files_are_the_parents(tx, baked):
    """the files of a run without --fill, byte for byte, against the bake's arrays written the way the command wrote them before the option existed"""
    from texir_code_amd import atlas, dist_util, gbuffer as GB, io_formats as IO
    root, d = baked["root"], baked["dirs"]["plain"]
    assert sorted(os.listdir(d)) == ["0.png", "hdr_texture.hdr"]
    IO._OBJ_CACHE.clear()
    obj = IO.load_obj(os.path.join(root, "vrproc", "hdr_texture", "out1.obj"))
    sc = tx.Scene(obj["vertices"], obj["indices"], IO.triangle_uvs_open3d(obj), np.zeros((2, 2, 3), np.float32), device=0)
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(sc, 64, 64, want_ids=True)
    order = dist_util.morton_order(torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32), 64)
    panos = np.stack([IO.read_hdr(os.path.join(root, "hdr", i, "ccm.hdr")) for i in baked["ids"]], 0)
    Wm, cam = atlas.camera_matrices(baked["E"])
    view, pix, rgb = atlas.bake_atlas(sc, pos, nrm, Wm, cam, panos, texel_ids=order)
    ref = str(baked["tmp"] / "parent")
    os.makedirs(ref)
    IO.write_hdr(os.path.join(ref, "hdr_texture.hdr"), rgb.reshape(64, 64, 3).cpu().numpy())
    IO.write_png(os.path.join(ref, "0.png"), np.ascontiguousarray(atlas.index_codes(view, pix, 32, 64).reshape(64, 64, 3)[..., ::-1]))
    for n in ("hdr_texture.hdr", "0.png"):
        assert open(os.path.join(d, n), "rb").read() == open(os.path.join(ref, n), "rb").read(), n


def test_end_to_end_fill(tx, baked):
    from texir_code_amd import atlas, conf as CF, datasets as D, dist_util, gbuffer as GB, io_formats as IO, models
    from texir_code_amd.trainer import exp_runner as ER
    root, dp, df = baked["root"], baked["dirs"]["plain"], baked["dirs"]["fill"]
    assert sorted(os.listdir(df)) == ["0.png", "atlas_fill.npz", "hdr_texture.hdr"]
    assert open(os.path.join(dp, "0.png"), "rb").read() == open(os.path.join(df, "0.png"), "rb").read()      # codes for observed texels only
    a = IO.read_hdr(os.path.join(dp, "hdr_texture.hdr")).reshape(-1, 3)
    b = IO.read_hdr(os.path.join(df, "hdr_texture.hdr")).reshape(-1, 3)
    src = np.load(os.path.join(df, "atlas_fill.npz"))["src"]
    assert src.shape == (64, 64) and src.dtype == np.int32
    src = src.reshape(-1)
    view, _ = atlas.decode_codes(IO.read_index_texture(os.path.join(df, "0.png")).reshape(-1, 3), 32, 64)
    IO._OBJ_CACHE.clear()
    obj = IO.load_obj(os.path.join(root, "vrproc", "hdr_texture", "out1.obj"))
    sc = tx.Scene(obj["vertices"], obj["indices"], IO.triangle_uvs_open3d(obj), np.zeros((2, 2, 3), np.float32), device=0)
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(sc, 64, 64, want_ids=True)
    cov = (prim.reshape(-1) >= 0).cpu().numpy()
    seen, hole = cov & (view >= 0), cov & (view < 0)
    filled, black = hole & (src >= 0), hole & (src < 0)
    print("covered %d: observed %d, filled %d, left black %d" % (cov.sum(), seen.sum(), filled.sum(), black.sum()))
    assert seen.sum() > 0.5 * cov.sum() and filled.sum() > 0.1 * hole.sum()
    au, bu = a.view(np.uint32), b.view(np.uint32)
    assert np.array_equal(bu[seen], au[seen])                              # observed texels keep their bits
    assert (src[~hole] == -1).all() and seen[src[filled]].all()
    assert np.array_equal(bu[filled], au[src[filled]])                     # every filled texel holds its source's bits
    assert not bu[black].any() and not au[hole].any()
    # the device's src is the rule's: the float32 restatement on the same G-buffer and lists
    order = dist_util.morton_order(torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32), 64).cpu().numpy()
    case = C.Case("e2e", pos.reshape(-1, 3).cpu().numpy(), nrm.reshape(-1, 3).cpu().numpy(), order[seen[order]], order[hole[order]], 0.5, 0.5)
    want = C.fill_f32(case, sentinel=(-1, 0.0))[0]
    assert np.array_equal(src, want)
    # every uncovered texel equals its uv-nearest covered texel
    rr, cc = np.nonzero(cov.reshape(64, 64))
    b3 = b.reshape(64, 64, 3)
    for r, c_ in zip(*np.nonzero(~cov.reshape(64, 64))):
        d2 = (rr - r) ** 2 + (cc - c_) ** 2
        near = d2 == d2.min()
        assert any(np.array_equal(b3[r, c_], b3[p, q]) for p, q in zip(rr[near], cc[near])), (r, c_)
    # both directories as datasets of their own: the 4-byte texel layout stays in force, and the fill only adds radiance
    irr = {}
    for key, d in (("plain", dp), ("fill", df)):
        root2 = os.path.dirname(os.path.dirname(d))
        shutil.copy(os.path.join(root, "vrproc", "hdr_texture", "out1.obj"), os.path.join(d, "out1.obj"))
        shutil.copytree(os.path.join(root, "info"), os.path.join(root2, "info"))
        conf_path = os.path.join(root2, "irt.conf")
        D.write_conf(conf_path, root2, cube_res=16, spp=(64, 16), model="irt")
        txt = open(conf_path).read()
        open(conf_path, "w").write(txt.replace("irt_res = native", "irt_res = native\n    texel_gbuffer = raster"))
        IO._OBJ_CACHE.clear()
        ER.main(["--conf", conf_path, "--trainstage", "IrrT", "--gpu", "0"])
        irr[key] = IO.read_hdr(os.path.join(d, "0_irr_texture.hdr")).reshape(-1, 3)
        scene, _, _ = models._load_scene(CF.ConfigFactory.parse_file(conf_path), 0)
        assert scene.texture_layout() >= 3, (key, scene.texture_layout())
    assert np.isfinite(irr["fill"]).all()
    m0, m1 = float(irr["plain"][cov].mean()), float(irr["fill"][cov].mean())
    print("mean irradiance over the covered texels: unfilled %.6f, filled %.6f" % (m0, m1))
    assert m1 >= m0 and (irr["fill"][hole].sum(-1) > 0).sum() >= (irr["plain"][hole].sum(-1) > 0).sum()
