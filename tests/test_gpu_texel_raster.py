"""GPU: the uv-space texel rasteriser (texir_texel_gbuffer, csrc/texraster.hip; gbuffer.raster_texel_gbuffer; train.texel_gbuffer = raster) against the float64
oracle, the integer restatement of the crack / overlap rules, the float32 restatement of the header and the synthetic generator's own G-buffer
(texel_raster_cases.py states every rule and bound; test_texel_raster_ref_cpu.py shows the checker rejects seven mutants).

Every texel of every case is checked: the chosen id is in the oracle's possible set (margin M = 2^-18) and not above the lowest certain id, certainly covered
texels are covered, texels without a possible coverer are all-zero seams, and bary / pos / nrm lie within the first-order bound (u = 2^-24, K = 4) around the
float64 values of the id the device chose.  The share of weak texels (possible, not certain) is asserted <= 2 % from the oracle before the device is asked.

NO MI355X RUN OF THIS MODULE IS RECORDED YET.  The float32 restatement of the header's arithmetic (texel_raster_cases.raster_f32), put in the device's place,
passes every check below on the CPU; its worst error / bound over all texels of the three general-position cases is bary 0.039, pos 0.22, nrm 0.21 (K = 4
included), and the stage-level IrT figure (raster route against file route, asserted < 1e-3 rel-L2) has not been observed.  DESIGN.md section 7 says the same.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import texel_raster_cases as C

pytestmark = pytest.mark.gpu


def _scene(tx, mesh, normals=True):
    from texir_code_amd import gbuffer as GB
    sc = tx.Scene(mesh.verts, mesh.tris, mesh.tri_uvs, np.zeros((2, 2, 3), np.float32), device=0)
    if normals and mesh.cnrm is not None:
        GB.set_corner_normals(sc, mesh.cnrm)
    return sc


def _run(sc, H, W, normal="geometric", offset=C.OFFSET):
    from texir_code_amd import gbuffer as GB
    pos, nrm, prim, bary = GB.raster_texel_gbuffer(sc, H, W, normal=normal, offset=offset, want_ids=True)
    torch.cuda.synchronize()
    return {"prim": prim.cpu().numpy(), "pos": pos.cpu().numpy(), "nrm": nrm.cpu().numpy(), "bary": bary.cpu().numpy()}


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


def test_entry_points_exist():
    from texir_code_amd import _lib, gbuffer as GB
    L = _lib.lib()
    assert hasattr(L, "texir_texel_gbuffer") and hasattr(L, "texir_texel_gbuffer_workspace_bytes")
    assert callable(GB.raster_texel_gbuffer)


def test_exact_cases_bit_for_bit(tx):
    """uvs on multiples of 2^-k, power-of-two atlases: every edge value is exact, so ownership must equal the integer statement of the rules -- centres on shared
    edges and on vertices where six (eight, four) triangles meet, mirrored charts, two charts overlapping, triangles smaller than a texel, one triangle over the
    whole atlas, uvs outside [0,1], zero-area and NaN triangles, H != W, sizes around lane and tile boundaries"""
    for mesh, H, W, k in C.exact_cases():
        own, count = C.raster_exact_int(mesh, H, W, k)
        out = _run(_scene(tx, mesh), H, W)
        assert np.array_equal(out["prim"], own), (mesh.name, H, W, int((out["prim"] != own).sum()))
        if "overlapping" not in mesh.name:
            assert count.max() <= 1                                      # exactly one owner per covered texel
        ref = C.raster_f32(mesh, H, W)
        assert np.array_equal(out["bary"].view(np.uint32), ref["bary"].view(np.uint32)), mesh.name      # exact edge values, one correctly rounded quotient
        seam = out["prim"] < 0
        assert not out["pos"][seam].any() and not out["nrm"][seam].any()


GENERAL = [("room", 2000, 128), ("room", 20000, 512), ("house", 20000, 512)]


@pytest.fixture(scope="module")
def general():
    cache = {}

    def get(style, T, res):
        key = (style, T, res)
        if key not in cache:
            mesh, sc = C.synth_mesh(style, T)
            C.margin_of(mesh)
            orc = C.Oracle(mesh, res, res)
            cache[key] = (mesh, sc, orc)
        return cache[key]
    return get


@pytest.mark.parametrize("style,T,res", GENERAL)
def test_general_position_against_oracle(tx, general, style, T, res):
    mesh, _, orc = general(style, T, res)
    share = orc.weak_share()
    print("%s %d %d^2: weak share %.4f of %d possibly covered texels" % (style, T, res, share, orc.any_possible.sum()))
    assert share <= C.CAP_WEAK                                            # from the oracle alone, before the device is consulted
    sc = _scene(tx, mesh)
    for normal in ("geometric", "shading"):
        out = _run(sc, res, res, normal)
        fails, worst = C.check_output(mesh, res, res, out, orc, normal)
        print("%s %d %d^2 %s: worst error / bound %s" % (style, T, res, normal, worst))
        assert not fails, fails
    # the device follows the header's arithmetic to the bit: ownership equals the numpy float32 restatement's
    ref = C.raster_f32(mesh, res, res)
    out = _run(sc, res, res)
    assert np.array_equal(out["prim"], ref["prim"]), int((out["prim"] != ref["prim"]).sum())


def test_odd_sizes_against_oracle(tx):
    for mesh, H, W in C.odd_size_cases():
        orc = C.Oracle(mesh, H, W)
        out = _run(_scene(tx, mesh), H, W)
        fails, _ = C.check_output(mesh, H, W, out, orc)
        assert not fails, (mesh.name, H, W, fails)
        assert np.array_equal(out["prim"], C.raster_f32(mesh, H, W)["prim"]), (mesh.name, H, W)


@pytest.mark.parametrize("style,T,res", GENERAL)
def test_against_the_synthetic_generator(tx, general, style, T, res):
    """pins orientation and crack-freedom on real chart meshes: coverage = make_texel_gbuffer's valid except within M of a chart rectangle's border (share
    <= 2 %); the surface point pos - offset * nrm agrees with the generator's within the derived bound of the device's own primitive plus what a uv
    distance of M moves the point (position is continuous across a shared edge: the owner does not matter); nrm = the geometric normal of the device's id"""
    from texir_code_amd import synth
    mesh, sc0, orc = general(style, T, res)
    pos_s, nrm_s, valid = synth.make_texel_gbuffer(sc0, res)
    pos_s, nrm_s, valid = pos_s[::-1].astype(np.float64), nrm_s[::-1].astype(np.float64), valid[::-1] > 0          # file orientation (datasets.write_synthetic_dataset)
    near = C.chart_border_texels(sc0, res, res)
    share = near.sum() / max(1, valid.sum())
    print("%s %d %d^2: %d texels within M of a chart border (%.4f)" % (style, T, res, near.sum(), share))
    assert share <= C.CAP_WEAK
    out = _run(_scene(tx, mesh), res, res)
    cov = out["prim"] >= 0
    assert np.array_equal(cov | near, valid | near), int(((cov != valid) & ~near).sum())
    both = cov & valid
    ref = C.attr_ref(mesh, res, res, out["prim"])
    uv = mesh.uv()[np.where(cov, out["prim"], 0)].astype(np.float64)
    P = mesh.P()[np.where(cov, out["prim"], 0)].astype(np.float64)
    S = np.abs(np.cross(uv[..., 1, :] - uv[..., 0, :], uv[..., 2, :] - uv[..., 0, :]))
    L1 = np.linalg.norm(uv[..., 0, :] - uv[..., 2, :], axis=-1); L2 = np.linalg.norm(uv[..., 1, :] - uv[..., 0, :], axis=-1)
    A, B = np.abs(P[..., 1, :] - P[..., 0, :]), np.abs(P[..., 2, :] - P[..., 0, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        slack = C.M * (A * (L1 / S)[..., None] + B * (L2 / S)[..., None])
    surf_d = out["pos"].astype(np.float64) - C.OFFSET * out["nrm"].astype(np.float64)
    surf_s = pos_s - 1e-2 * nrm_s
    bound = ref["dpos"] + C.OFFSET * ref["dnrm"] + 4 * C.U * (np.abs(pos_s) + C.OFFSET) + slack
    err = np.abs(surf_d - surf_s)
    bad = both[..., None] & ~(err <= bound)
    assert not bad.any(), (int(bad.any(-1).sum()), float(err[bad].max()))
    nerr = np.abs(out["nrm"].astype(np.float64) - ref["ngeo"])
    assert not (cov[..., None] & ~(nerr <= ref["dnrm"])).any()
    # the generator's normal is the same face's (same winding) wherever the centre is not within M of an interior edge.  It is computed from the chart's grid
    # cell, the device's from the triangle, which the generator's fix-up may have split at an edge midpoint rounded to float32: the vertex moves by u |P| over
    # triangle heights of at least 1e-3 |P| at these sizes, an angle below 1e-4 -- the cosine is within 1e-6 of 1
    sure = both & (orc.n_possible == 1)
    assert sure.sum() > 0.9 * both.sum()
    assert ((out["nrm"].astype(np.float64) * nrm_s).sum(-1)[sure] > 1.0 - 1e-6).all()


def test_two_runs_same_bits_and_triangle_order_does_not_matter(tx, general):
    mesh, _, orc = general("room", 20000, 512)
    sc = _scene(tx, mesh)
    a, b = _run(sc, 512, 512), _run(sc, 512, 512)
    assert _same_bits(a, b)
    perm = np.random.default_rng(5).permutation(mesh.T)
    c = _run(_scene(tx, mesh.permuted(perm)), 512, 512)
    one = orc.n_possible == 1                                             # no overlap, not even within the margin
    assert one.sum() > 0.5 * (a["prim"] >= 0).sum()
    assert np.array_equal(perm[np.where(c["prim"] >= 0, c["prim"], 0)][one], np.where(a["prim"] >= 0, a["prim"], perm[0])[one])
    for k in ("pos", "nrm", "bary"):
        assert np.array_equal(a[k].view(np.uint32)[one], c[k].view(np.uint32)[one]), k


def test_graph_capture_and_replay(tx, general):
    """no allocation, no synchronisation: the entry point records into a graph; the replay writes the eager run's bits"""
    from texir_code_amd import _lib
    mesh, _, _ = general("room", 2000, 128)
    sc = _scene(tx, mesh)
    H = W = 128
    want = _run(sc, H, W, "shading")
    L = _lib.lib()
    nb = ctypes.c_int64()
    _lib.check(L.texir_texel_gbuffer_workspace_bytes(sc.h, H, W, ctypes.byref(nb)))
    ws = torch.empty(nb.value, device="cuda", dtype=torch.uint8)
    pos, nrm = torch.zeros(H, W, 3, device="cuda"), torch.zeros(H, W, 3, device="cuda")
    prim, bary = torch.zeros(H, W, device="cuda", dtype=torch.int32), torch.zeros(H, W, 2, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_texel_gbuffer(sc.h, H, W, 1, C.OFFSET, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(prim), _lib.ptr(bary), _lib.ptr(ws), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for t in (pos, nrm, prim, bary):
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        got = {"prim": prim.long().cpu().numpy(), "pos": pos.cpu().numpy(), "nrm": nrm.cpu().numpy(), "bary": bary.cpu().numpy()}
        assert _same_bits(got, want)


def test_argument_errors(tx, general):
    from texir_code_amd import _lib, gbuffer as GB
    mesh, _, _ = general("room", 2000, 128)
    sc = _scene(tx, mesh, normals=False)
    with pytest.raises(_lib.TexirError, match="corner_normals"):
        GB.raster_texel_gbuffer(sc, 16, 16, normal="shading")
    with pytest.raises(_lib.TexirError, match="16384"):
        GB.raster_texel_gbuffer(sc, 0, 16)
    with pytest.raises(ValueError):
        GB.raster_texel_gbuffer(sc, 16, 16, normal="smooth")
    pos, nrm = GB.raster_texel_gbuffer(sc, 16, 24)                         # ids are optional
    assert pos.shape == (16, 24, 3) and nrm.shape == (16, 24, 3)


def _irrt(conf_path):
    from texir_code_amd import io_formats as IO
    from texir_code_amd.trainer import exp_runner as ER
    IO._OBJ_CACHE.clear()
    ER.main(["--conf", conf_path, "--trainstage", "IrrT", "--gpu", "0"])


def test_stage_raster_route(tmp_path):
    """--trainstage IrrT with train.texel_gbuffer = raster on a copy of a synthetic dataset WITHOUT 0.png and texel_gbuffer.npz writes 0_irr_texture.hdr; the IrT
    equals the file route's within the existing IrT tolerance (1e-3 rel-L2) on the texels valid in both; a default conf and an explicit `file` conf write the
    same bytes (the default route is untouched); without 0.png a non-integer train.irt_res is an error that names the key"""
    from texir_code_amd import datasets as D, io_formats as IO
    from conftest import rel_l2
    root = str(tmp_path / "data")
    D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
    conf_file = str(tmp_path / "irt.conf")
    D.write_conf(conf_file, root, cube_res=16, spp=(64, 16), model="irt")
    base = open(conf_file).read()
    assert "irt_res = native" in base and "texel_gbuffer" not in base
    hdr = os.path.join(root, "vrproc", "hdr_texture", "0_irr_texture.hdr")
    _irrt(conf_file)
    bytes_default = open(hdr, "rb").read()
    irt_file = IO.read_hdr(hdr)
    os.remove(hdr)
    conf_explicit = str(tmp_path / "irt_file.conf")
    open(conf_explicit, "w").write(base.replace("irt_res = native", "irt_res = native\n    texel_gbuffer = file"))
    _irrt(conf_explicit)
    assert open(hdr, "rb").read() == bytes_default

    root2 = str(tmp_path / "data_raster")
    shutil.copytree(root, root2)
    mesh2 = os.path.join(root2, "vrproc", "hdr_texture")
    for f in ("0.png", "texel_gbuffer.npz", "0_irr_texture.hdr"):
        os.remove(os.path.join(mesh2, f))
    conf_r = str(tmp_path / "irt_raster.conf")
    open(conf_r, "w").write(base.replace(root, root2).replace("irt_res = native", "irt_res = 64\n    texel_gbuffer = raster"))
    _irrt(conf_r)
    irt_r = IO.read_hdr(os.path.join(mesh2, "0_irr_texture.hdr"))
    assert irt_r.shape == irt_file.shape == (64, 64, 3)
    both = (irt_r.sum(-1) != 0) & (irt_file.sum(-1) != 0)
    assert both.sum() > 0.95 * max((irt_r.sum(-1) != 0).sum(), (irt_file.sum(-1) != 0).sum())
    err = rel_l2(irt_r[both], irt_file[both])
    print("IrT raster vs file route: rel-L2 %.3e on %d texels valid in both" % (err, both.sum()))
    assert err < 1e-3

    conf_bad = str(tmp_path / "irt_bad.conf")
    open(conf_bad, "w").write(base.replace(root, root2).replace("irt_res = native", "irt_res = native\n    texel_gbuffer = raster"))
    with pytest.raises(ValueError, match="train.irt_res"):
        _irrt(conf_bad)
    # shading normals through the stage: runs and differs from the geometric route only slightly on this mesh
    conf_s = str(tmp_path / "irt_shading.conf")
    open(conf_s, "w").write(base.replace(root, root2).replace("irt_res = native", "irt_res = 64\n    texel_gbuffer = raster\n    texel_normal = shading"))
    _irrt(conf_s)
    assert IO.read_hdr(os.path.join(mesh2, "0_irr_texture.hdr")).shape == (64, 64, 3)


def test_cli_writes_the_file_routes_npz(tmp_path):
    from texir_code_amd import datasets as D, tools
    root = str(tmp_path / "data")
    D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=1)
    mesh_dir = os.path.join(root, "vrproc", "hdr_texture")
    want = np.load(os.path.join(mesh_dir, "texel_gbuffer.npz"))
    dst = str(tmp_path / "out.npz")
    assert tools.main(["texel-gbuffer", os.path.join(mesh_dir, "out1.obj"), "64", dst]) == 0
    got = np.load(dst)
    assert got["position"].shape == want["position"].shape and got["position"].dtype == np.float32
    v = (want["normal"] != 0).any(-1) & (got["normal"] != 0).any(-1)
    assert v.sum() > 0.95 * (want["normal"] != 0).any(-1).sum()
    # surface points (the normal of a centre on a cell's diagonal may be either face's; the point is the same): float32 rounding of a 5-unit room is ~1e-6
    surf = lambda z: z["position"].astype(np.float64) - 1e-2 * z["normal"].astype(np.float64)
    assert np.abs(surf(got)[v] - surf(want)[v]).max() < 1e-4
