"""No GPU: the float64 reference of the atlas bake's rule (atlas_bake_cases.py) is sharp and its checker has teeth, the camera-frame convention of
atlas.camera_matrices is the one Pano2Cube and cameras.cube_mvps share, and the index codes are the reference's.

(a) the float32 numpy restatement of the kernel's arithmetic (header's operation sequence + trace_cases.trace_f32) passes the checker on every case, and the
    checker rejects seven mutants;  (b) at most 3 % of a case's listed texels have more than one admissible outcome;  (c) the convention pin;
(d) decode_codes(index_codes(.)) is the identity for h, w up to 8000;  (e) the gather through the codes is tools/trans_hdr_tex.py:27-57's.
"""
import numpy as np
import pytest
import torch

import atlas_bake_cases as C


@pytest.mark.parametrize("name", C.ALL)
def test_caps(name):
    """(b), from the reference alone"""
    ref = C.case(name).ref()
    print(name, ref.stats())
    assert ref.caps() <= C.CAP_MULTI, ref.stats()
    if name == "closed_box":
        assert ref.none_ok.all() and not ref.view_ok.any()                   # nobody sees the texels inside: -1 is the only admissible outcome
    if name == "pole":
        i = ref.row_of[0]
        assert len(ref.cols[i][0]) == C.case(name).w                         # the column is unconstrained straight under the camera
    if name == "tie":
        assert ref.twin[:, 0, 1].all() and ref.certain[:, :2].all()          # every texel ties exactly between views 0 and 1 ...
        assert ref.view_ok[:, 0].all() and not ref.view_ok[:, 1].any()       # ... and only the lower id is admissible


def test_reference_table():
    """the figures the rule was designed against: the room at 64^2 with 2 x 2 views of 32 x 64, at 96^2 with 3 x 3 views of 50 x 100"""
    a, b = C.case("room64").ref().stats(), C.case("room96").ref().stats()
    assert a["texels"] == 3052 and abs(a["got_a_view"] - 0.598) < 5e-4 and a["two_views"] == 0 and a["uncertain_vis"] == 0
    assert b["texels"] == 6904 and abs(b["got_a_view"] - 0.720) < 5e-4 and b["two_views"] == 0 and b["uncertain_vis"] == 0


@pytest.mark.parametrize("name", C.ALL)
def test_float32_restatement_passes(name):
    """(a)"""
    case = C.case(name)
    sentinel = (-7, 5, 0.25)
    view, pix, rgb, stats = C.bake_f32(case, sentinel=sentinel)
    fails = C.check(case, view, pix, rgb, sentinel=sentinel)
    assert not fails, (len(fails), fails[:5])
    assert stats[3] == int((view[case.ref().tex] >= 0).sum()) and stats[2] >= stats[3] and stats[0] >= stats[1] >= stats[2]


@pytest.mark.parametrize("mut", C.MUTANTS)
def test_checker_rejects_mutant(mut):
    case = C.case(C.MUTANT_CASES[mut])
    view, pix, rgb, _ = C.bake_f32(case, mut)
    fails = C.check(case, view, pix, rgb)
    print(mut, len(fails), fails[:1])
    assert fails


def test_wrong_rgb_is_rejected():
    case = C.case("list64")
    view, pix, rgb, _ = C.bake_f32(case)
    t = int(case.ref().tex[np.nonzero(view[case.ref().tex] >= 0)[0][0]])
    rgb[t, 2] = np.nextafter(rgb[t, 2], np.float32(1e9))
    assert C.check(case, view, pix, rgb)


def _face_points(mvp, c, centres, depth=2.0):
    """world-space points of the face pixels of cameras.cube_mvps' six faces (float64): pixel (row i, col j) at ndc (g[j], g[i]) (texir_gbuffer_cast's
    layout), g = the pixel centres, or Pano2Cube's own corner-aligned sample positions linspace(-1, 1, c)"""
    from texir_code_amd import cameras
    proj = cameras.projection().astype(np.float64)
    g = ((np.arange(c) + 0.5) / c * 2 - 1) if centres else np.linspace(-1.0, 1.0, c)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    clip = np.stack([xx * depth, yy * depth, np.full_like(xx, depth), np.ones_like(xx)], -1) @ proj.T
    return np.stack([(clip @ np.linalg.inv(mvp[f].double().numpy()))[..., :3] for f in range(6)], 0)


def pin_agreement(points, Wk, h, w, c):
    """share of face pixels at which Pano2Cube.Tocube(nearest) shows the pixel pano_pixel names for the face pixel's world point, and the largest offset"""
    from texir_code_amd import atlas
    from texir_code_amd.pano2cube import Pano2Cube
    pano = torch.zeros(1, 2, h, w)
    r, cc = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pano[0, 0], pano[0, 1] = r, cc                                           # every pixel carries its own (row, col)
    cube = Pano2Cube(1, w, h, c, 2).Tocube(pano, "nearest")[0].reshape(6, 2, c, c)
    row, col = atlas.pano_pixel(Wk, torch.as_tensor(points, dtype=torch.float64), h, w)
    dr = (row - cube[:, 0].long()).abs()
    dc = (col - cube[:, 1].long()).abs()
    dc = torch.minimum(dc, w - dc)                                           # (the azimuth wraps)
    per_face = ((dr == 0) & (dc == 0)).float().reshape(6, -1).mean(1)
    return float(((dr == 0) & (dc == 0)).float().mean()), int(torch.maximum(dr, dc).max()), per_face.tolist()


def test_convention_pin():
    """(c): a rotated, translated extrinsic; the face pixels' world points come from cube_mvps (inverted), sampled where Pano2Cube samples; the panorama
    pixel Pano2Cube shows there is the one pano_pixel(camera_matrices(E)) names: >= 99 % exactly, the rest one pixel off (nearest-rounding ties and
    Pano2Cube's float32 grid)"""
    from texir_code_amd import atlas, cameras
    rng = np.random.default_rng(5)
    E = np.eye(4)
    E[:3, :3] = C.random_rotation(rng)
    E[:3, 3] = (1.5, 0.7, -2.0)
    mvp, cam = cameras.cube_mvps(E.astype(np.float32))
    Wm, cp = atlas.camera_matrices(E[None])
    assert np.allclose(cp[0].numpy(), cam.numpy())
    c, h, w = 32, 37, 90
    share, worst, per_face = pin_agreement(_face_points(mvp, c, centres=False), Wm[0], h, w, c)
    print("convention pin: %.4f of the face pixels agree, worst offset %d px, per face %s" % (share, worst, per_face))
    assert share >= 0.99 and worst <= 1 and min(per_face) >= 0.98
    # a wrong convention is far from passing: y not flipped, or x mirrored
    for S in (np.diag([1.0, -1.0, 1.0]), np.diag([-1.0, 1.0, 1.0])):
        bad = torch.from_numpy(S) @ Wm[0].double()
        assert pin_agreement(_face_points(mvp, c, centres=False), bad, h, w, c)[0] < 0.6


def test_pixel_centres_against_the_grid():
    """the sizes of the device pin (test_gpu_atlas_bake.py): texir_gbuffer_cast samples pixel CENTRES, Pano2Cube corner-aligned positions linspace(-1, 1, c),
    up to half a face pixel apart; at c = 128 against a 5 x 12 panorama the two sample positions alone (float64, no kernel) name the same panorama pixel
    for >= 99 % of the face pixels"""
    from texir_code_amd import atlas, cameras
    E = np.stack(cameras.grid_cameras(2), 0).astype(np.float64)
    Wm, _ = atlas.camera_matrices(E)
    mvp, _ = cameras.cube_mvps(E[1].astype(np.float32))
    share, worst, _ = pin_agreement(_face_points(mvp, 128, centres=True), Wm[1], 5, 12, 128)
    print("pixel centres against Pano2Cube's grid at c = 128, 5 x 12: %.4f, worst %d" % (share, worst))
    assert share >= 0.995 and worst <= 1


def test_codes_round_trip():
    """(d)"""
    from texir_code_amd import atlas
    for n in list(range(1, 70)) + [90, 100, 512, 1000, 1024, 2048, 4000, 4096, 7999, 8000]:
        i = np.arange(n)
        codes = atlas.index_codes(np.zeros(n, np.int64), np.stack([i, i[::-1]], -1), n, n)
        assert codes.dtype == np.uint16 and codes[..., :2].min() >= 1 and codes[..., :2].max() <= 50000
        view, pix = atlas.decode_codes(codes, n, n)
        assert (view == 0).all() and (pix[:, 0] == i).all() and (pix[:, 1] == i[::-1]).all(), n
    codes = atlas.index_codes(np.array([-1, 3]), np.array([[5, 6], [7, 15]]), 8, 16)
    assert not codes[0].any() and codes[1, 2] == 3
    view, pix = atlas.decode_codes(codes, 8, 16)
    assert view.tolist() == [-1, 3] and pix.tolist() == [[0, 0], [7, 15]]


def _repack_hdr(idx, panos):
    """tools/trans_hdr_tex.py:27-57 (repackHDRTexture) on arrays: idx [H,W,3] = (row code, col code, panorama id) as cv2 reads 0.png"""
    out = np.zeros(idx.shape, np.float32)
    for k in np.unique(idx[:, :, 2]):
        rows, cols = np.where(idx[:, :, 2] == k)
        hdr = panos[k]
        height, width, _ = hdr.shape
        pc = np.clip((idx[rows, cols, 1] / 50000 * width).astype(int), 0, width - 1)
        pr = np.clip((idx[rows, cols, 0] / 50000 * height).astype(int), 0, height - 1)
        out[rows, cols, :] = hdr[pr, pc, :3]
        hs, ws = np.where((idx[:, :, 0] + idx[:, :, 1] + idx[:, :, 2]) == 0)
        out[hs, ws] = 0
    return out


def test_gather_through_the_codes_is_the_reference_repack():
    """(e): rgb of the bake == repackHDRTexture through index_codes(view, pix), bit for bit; seams are zero"""
    from texir_code_amd import atlas
    case = C.case("room64_rot")
    rng = np.random.default_rng(3)
    panos = rng.uniform(0.01, 30.0, (case.K, case.h, case.w, 3)).astype(np.float32)
    view, pix, _, _ = C.bake_f32(case, sentinel=(-1, 0, 0.0))
    got = view >= 0
    rgb = np.zeros((case.Nt, 3), np.float32)
    rgb[got] = panos[view[got], pix[got, 0], pix[got, 1]]
    codes = atlas.index_codes(view, pix, case.h, case.w).reshape(64, 64, 3)
    out = _repack_hdr(codes, panos)
    assert got.sum() > 1000
    assert np.array_equal(out.reshape(-1, 3).view(np.uint32), rgb.view(np.uint32))
    assert not out.reshape(-1, 3)[~got].any()


def test_cli_bad_arguments_and_no_overwrite(tmp_path):
    """decided before anything touches a device: a malformed size or cosine is refused, and so is a directory that already holds one of the files"""
    from texir_code_amd import tools
    root = str(tmp_path / "data")
    out = tmp_path / "out"
    out.mkdir()
    assert tools.main(["bake-atlas", root, "12y"]) == 2
    assert tools.main(["bake-atlas", root, "64", "--cos-min", "high"]) == 2
    assert tools.main(["bake-atlas", root, "64", "--normal", "smooth"]) == 2
    (out / "0.png").write_bytes(b"kept")
    assert tools.main(["bake-atlas", root, "64x32", "--out", str(out)]) == 1
    assert (out / "0.png").read_bytes() == b"kept"
