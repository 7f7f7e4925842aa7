"""GPU: the pad + denoise step between the stages (csrc/texpost.hip behind texir_texture_pad / texir_texture_denoise, texir_code_amd/texpost.py, and the
IrrT runner's train.irt_pad / train.irt_denoise keys).  The nearest-texel transform is checked against brute force on EVERY hole, the `reference` mode
against the CPU tool it restates, the filter against tools.denoise_atrous on the CPU."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from texpost_cases import brute_force, hole_mask, noisy_lowpass, seeded_guides, seeded_image

pytestmark = pytest.mark.gpu

SIZES = [(96, 128), (100, 124)]


def _cpu_denoise(img, **kw):
    """tools.denoise_atrous on the CPU, on ONE host thread: the images are small and the filter is thousands of tiny elementwise torch ops, each of
    which would otherwise be a parallel region over every core the box shows (same values: nothing in it reduces across threads)"""
    from texir_code_amd import tools
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return tools.denoise_atrous(img, device="cpu", **kw)
    finally:
        torch.set_num_threads(n)


def _pad(img, mode="nearest"):
    from texir_code_amd import texpost
    out, src = texpost.pad_texture(torch.from_numpy(img).cuda(), mode=mode, return_src=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), src.cpu().numpy()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_nearest_mode_every_hole_takes_a_texel_at_minimal_distance(h, w):
    img, valid = seeded_image(h, w)
    out, src = _pad(img)
    hole = hole_mask(img)
    assert np.array_equal(hole, ~valid)
    hy, hx, vy, vx, d2, dmin = brute_force(img)
    assert len(hy) > 5000
    # src names a valid texel at exactly the minimal squared distance, for every hole
    sy, sx = src[hy, hx] // w, src[hy, hx] % w
    assert not hole[sy, sx].any()
    assert np.array_equal((sy - hy).astype(np.int64) ** 2 + (sx - hx).astype(np.int64) ** 2, dmin)
    # the output triple equals the value of SOME valid texel at minimal distance (checked on the values, not through src)
    vals = img[vy, vx]                                            # [n_valid, 3]
    ok = np.zeros(len(hy), bool)
    for i in range(len(hy)):
        cand = vals[d2[i] == dmin[i]]
        ok[i] = (cand == out[hy[i], hx[i]]).all(-1).any()
    assert ok.all(), "%d holes did not receive a minimal-distance value" % (~ok).sum()
    assert np.array_equal(out, img.reshape(-1, 3)[src.reshape(-1)].reshape(h, w, 3))
    assert np.array_equal(src[~hole], np.arange(h * w).reshape(h, w)[~hole])
    assert out[~hole].tobytes() == img[~hole].tobytes()
    assert not (out.sum(-1) == 0).any()
    out2, src2 = _pad(img)
    assert out2.tobytes() == out.tobytes() and src2.tobytes() == src.tobytes()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_reference_mode_every_hole_and_the_cpu_tool(h, w):
    from texir_code_amd import texpost
    img, _ = seeded_image(h, w)
    out, src = _pad(img, "reference")
    hole = hole_mask(img)
    hy, hx, vy, vx, d2, dmin = brute_force(img)
    rm, cm = texpost.reference_index_map(h), texpost.reference_index_map(w)
    rr, cc = rm[vy], cm[vx]
    okmap = (rr >= 0) & (cc >= 0)
    vals = np.where(okmap[:, None], img[np.maximum(rr, 0), np.maximum(cc, 0)], np.float32(0))        # what each valid source (r, c) yields in this mode
    ok = np.zeros(len(hy), bool)
    for i in range(len(hy)):
        cand = vals[d2[i] == dmin[i]]
        ok[i] = (cand == out[hy[i], hx[i]]).all(-1).any()
    assert ok.all(), "%d holes are not img[row_map[r], col_map[c]] of a minimal-distance texel" % (~ok).sum()
    assert out[~hole].tobytes() == img[~hole].tobytes()
    # the sources are the same exact transform as in nearest mode
    assert np.array_equal(src, _pad(img, "nearest")[1])
    # against the CPU tool (scipy + grid_sample): every non-hole and every hole whose nearest texel is unique; ties are scipy's own rule
    pytest.importorskip("scipy")
    from texir_code_amd import tools
    ref = tools.padding_texture(img)
    assert out[~hole].tobytes() == ref[~hole].tobytes()
    unique = (d2 == dmin[:, None]).sum(1) == 1
    share = unique.mean()
    print("reference mode %dx%d: %d holes, %.1f %% compared (unique nearest texel)" % (h, w, len(hy), 100 * share))
    assert share >= 0.75, "vacuous: only %.1f %% of the holes compared" % (100 * share)
    assert out[hy[unique], hx[unique]].tobytes() == ref[hy[unique], hx[unique]].tobytes()
    black = (out[hy, hx].sum(-1) == 0).mean()
    assert 0.25 < black < 0.45                                # the rounding accident is reproduced, not repaired


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_and_rules():
    from texir_code_amd import texpost
    rng = np.random.default_rng(7)
    # all valid: identity
    img = (rng.random((17, 23, 3)) + 0.5).astype(np.float32)
    out, src = _pad(img)
    assert out.tobytes() == img.tobytes() and np.array_equal(src.reshape(-1), np.arange(17 * 23))
    # all holes: copy, src = -1 (the (1, -1, 0) rule makes non-zero holes)
    img = np.zeros((9, 31, 3), np.float32)
    img[2, 3] = (1.0, -1.0, 0.0)
    for mode in texpost.MODES:
        out, src = _pad(img, mode)
        assert out.tobytes() == img.tobytes() and (src == -1).all()
    # one single valid texel
    img = np.zeros((33, 70, 3), np.float32)
    img[30, 5] = (0.5, 1.5, 2.5)
    out, src = _pad(img)
    assert (src == 30 * 70 + 5).all() and (out == img[30, 5]).all()
    # 1 x W and H x 1
    for shape in ((1, 77), (77, 1)):
        img = np.zeros(shape + (3,), np.float32)
        line = img.reshape(-1, 3)
        line[10], line[50] = 1.0, 2.0
        out, src = _pad(img)
        want = np.where(np.abs(np.arange(77) - 10) <= np.abs(np.arange(77) - 50), 10, 50)
        want[30] = src.reshape(-1)[30]                                   # the one tie (distance 20 both ways): either
        assert src.reshape(-1)[30] in (10, 50)
        assert np.array_equal(src.reshape(-1), want) and np.array_equal(out.reshape(-1, 3), line[want])
    # C = 1 .. 4
    for C in (1, 2, 4):
        img = (rng.random((20, 36, C)) + 0.5).astype(np.float32) * (rng.random((20, 36, 1)) < 0.3)
        out, src = _pad(img)
        hole = hole_mask(img)
        assert hole.any() and not hole_mask(out).any()
        assert np.array_equal(out, img.reshape(-1, C)[src.reshape(-1)].reshape(20, 36, C))
        yy, xx = np.nonzero(hole)
        vy, vx = np.nonzero(~hole)
        dmin = ((yy[:, None] - vy[None]) ** 2 + (xx[:, None] - vx[None]) ** 2).min(1)
        s = src[yy, xx]
        assert np.array_equal((s // 36 - yy) ** 2 + (s % 36 - xx) ** 2, dmin)
    # (1, -1, 0) is a hole and gets filled; (1, -1, 0.5) is not
    img = np.zeros((8, 8, 3), np.float32)
    img[4, 4] = (0.25, 0.5, 0.75)
    img[4, 5] = (1.0, -1.0, 0.0)
    img[0, 0] = (1.0, -1.0, 0.5)
    out, src = _pad(img)
    assert (out[4, 5] == img[4, 4]).all() and src[4, 5] == 4 * 8 + 4 and src[0, 0] == 0 and (out[0, 0] == img[0, 0]).all()
    # far: no window would cover this -- only columns 0..2 are valid, every source lies in column 2 of the hole's own row, up to 297 texels away
    img = np.zeros((40, 300, 3), np.float32)
    img[:, :3] = (rng.random((40, 3, 3)) + 0.5).astype(np.float32)
    out, src = _pad(img)
    rows = np.arange(40)[:, None]
    assert np.array_equal(src[:, 3:], np.broadcast_to(rows * 300 + 2, (40, 297)))
    assert np.array_equal(out[:, 3:], np.broadcast_to(img[:, 2:3], (40, 297, 3)))


def test_argument_errors():
    from texir_code_amd import _lib, texpost
    L = _lib.lib()
    H, W = 8, 12
    img = torch.rand(H, W, 3, device="cuda")
    out = torch.empty_like(img)
    tmp = torch.empty_like(img)
    ws = torch.empty(int(L.texir_texture_pad_workspace_bytes(H, W)), dtype=torch.uint8, device="cuda")
    rm = torch.zeros(H, dtype=torch.int32, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()

    def invalid(rc, word):
        assert rc == -1, rc                                    # TEXIR_ERR_INVALID
        msg = L.texir_last_error().decode()
        assert word in msg, msg

    invalid(L.texir_texture_pad(p(img), H, W, 5, None, None, p(out), None, p(ws), st), "C must be 1..4")
    invalid(L.texir_texture_pad(p(img), H, W, 0, None, None, p(out), None, p(ws), st), "C must be 1..4")
    invalid(L.texir_texture_pad(p(img), H, W, 3, p(rm), None, p(out), None, p(ws), st), "row_map and col_map")
    invalid(L.texir_texture_pad(p(img), H, W, 3, None, p(rm), p(out), None, p(ws), st), "row_map and col_map")
    invalid(L.texir_texture_pad(p(img), H, W, 3, None, None, p(img), None, p(ws), st), "out must not be img")
    invalid(L.texir_texture_pad(None, H, W, 3, None, None, p(out), None, p(ws), st), "null")
    invalid(L.texir_texture_pad(p(img), H, W, 3, None, None, None, None, p(ws), st), "null")
    invalid(L.texir_texture_pad(p(img), H, W, 3, None, None, p(out), None, None, st), "null")
    f = ctypes.c_float
    invalid(L.texir_texture_denoise(p(img), H, W, None, None, 0, f(0.5), f(0.3), f(0.25), p(tmp), p(out), st), "iterations must be 1..6")
    invalid(L.texir_texture_denoise(p(img), H, W, None, None, 7, f(0.5), f(0.3), f(0.25), p(tmp), p(out), st), "iterations must be 1..6")
    invalid(L.texir_texture_denoise(p(img), H, W, None, None, 3, f(0.5), f(0.3), f(0.25), p(tmp), p(img), st), "different buffers")
    invalid(L.texir_texture_denoise(None, H, W, None, None, 3, f(0.5), f(0.3), f(0.25), p(tmp), p(out), st), "null")
    invalid(L.texir_texture_denoise(p(img), H, W, None, None, 3, f(0.5), f(0.3), f(0.25), None, p(out), st), "null")
    # the Python layer raises TexirError (no CPU fallback) and rejects host tensors and unknown modes
    with pytest.raises(_lib.TexirError):
        texpost.pad_texture(torch.rand(4, 4, 5, device="cuda"))
    with pytest.raises(_lib.TexirError):
        texpost.pad_texture(torch.rand(4, 4, 3))
    with pytest.raises(_lib.TexirError):
        texpost.denoise(img, iterations=9)
    with pytest.raises(ValueError):
        texpost.pad_texture(img, mode="closest")


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(2048, 2048), (1536, 2048)])
def test_size_sampled_holes_against_a_window_scan(h, w):
    img, valid = seeded_image(h, w, cell=64)
    out, src = _pad(img)
    hole = ~valid
    assert not (out.sum(-1) == 0).any()
    assert np.array_equal(out, img.reshape(-1, 3)[src.reshape(-1)].reshape(h, w, 3))
    assert np.array_equal(src[valid], np.arange(h * w).reshape(h, w)[valid])
    hy, hx = np.nonzero(hole)
    pick = torch.randperm(len(hy), generator=torch.Generator().manual_seed(11))[:4096].numpy()
    deepest = 0
    for y, x in zip(hy[pick], hx[pick]):
        s = int(src[y, x])
        sy, sx = divmod(s, w)
        assert valid[sy, sx]
        d2 = (sy - y) ** 2 + (sx - x) ** 2
        r = int(math.ceil(math.sqrt(d2)))
        deepest = max(deepest, d2)
        y0, y1, x0, x1 = max(0, y - r), min(h, y + r + 1), max(0, x - r), min(w, x + r + 1)
        win = valid[y0:y1, x0:x1]
        yy, xx = np.nonzero(win)
        assert len(yy) and int(((yy + y0 - y) ** 2 + (xx + x0 - x) ** 2).min()) == d2, (y, x, d2)
    print("size %dx%d: %d holes, deepest sampled hole %.1f texels" % (h, w, len(hy), math.sqrt(deepest)))
    assert deepest >= 10 ** 2                                  # holes tens of texels deep were really exercised


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
BOUND = 1e-3          # the project's bound for float paths


@pytest.mark.parametrize("h,w,it", [(192, 256, 3), (160, 96, 4)])
def test_colour_only_denoise_against_the_torch_path(h, w, it, monkeypatch):
    from texir_code_amd import texpost
    img = noisy_lowpass(h, w)
    hole = hole_mask(img)
    assert 0.05 < hole.mean() < 0.15
    ref = _cpu_denoise(img, iterations=it)
    dev = torch.from_numpy(img).cuda()
    got = texpost.denoise(dev, iterations=it).cpu().numpy()
    err = rel_l2(got, ref)
    print("colour-only denoise %dx%d, %d passes: rel L2 vs the torch path (CPU) = %.3e (bound %.0e)" % (h, w, it, err, BOUND))
    assert (got[hole] == 0).all()
    assert np.isfinite(got).all() and err <= BOUND
    assert rel_l2(got, img) > 1e-2                              # it filtered
    # the two tap forms (LDS tile / global loads) are the same arithmetic in the same order
    for n in ("0", "3"):
        monkeypatch.setenv("TEXIR_ATROUS_LDS_PASSES", n)
        assert texpost.denoise(dev, iterations=it).cpu().numpy().tobytes() == got.tobytes(), n


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_guided_denoise(monkeypatch):
    from texir_code_amd import texpost
    h, w = 192, 256
    img = noisy_lowpass(h, w)
    nrm, pos = seeded_guides(h, w)
    dev = lambda a: torch.from_numpy(a).cuda()
    sig = (0.5, 0.3, 0.25)
    ref = _cpu_denoise(img, guide_nrm=nrm, guide_pos=pos, sigma_c=sig[0], sigma_n=sig[1], sigma_p=sig[2])
    got = texpost.denoise(dev(img), nrm=dev(nrm), pos=dev(pos), sigma=sig).cpu().numpy()
    err = rel_l2(got, ref)
    print("guided denoise %dx%d: rel L2 vs the guided torch path (CPU) = %.3e (bound %.0e)" % (h, w, err, BOUND))
    assert (got[hole_mask(img)] == 0).all() and err <= BOUND
    plain = texpost.denoise(dev(img)).cpu().numpy()
    assert rel_l2(got, plain) > 1e-3                            # the guides changed something
    for n in ("0", "3"):
        monkeypatch.setenv("TEXIR_ATROUS_LDS_PASSES", n)
        assert texpost.denoise(dev(img), nrm=dev(nrm), pos=dev(pos), sigma=sig).cpu().numpy().tobytes() == got.tobytes(), n
    monkeypatch.delenv("TEXIR_ATROUS_LDS_PASSES")
    # one guide alone (the other NULL or switched off by sigma 0)
    ref_n = _cpu_denoise(img, guide_nrm=nrm)
    assert rel_l2(texpost.denoise(dev(img), nrm=dev(nrm)).cpu().numpy(), ref_n) <= BOUND
    assert texpost.denoise(dev(img), nrm=dev(nrm), pos=dev(pos), sigma=(0.5, 0.3, 0.0)).cpu().numpy().tobytes() == texpost.denoise(dev(img), nrm=dev(nrm)).cpu().numpy().tobytes()
    # identity 1: constant guides = the colour-only kernel (which test 5 ties to the torch path as it was)
    const = np.broadcast_to(np.array([0.3, -0.2, 0.9], np.float32), (h, w, 3)).copy()
    e1 = rel_l2(texpost.denoise(dev(img), nrm=dev(const), pos=dev(const)).cpu().numpy(), plain)
    # identity 2: orthogonal normals on the two halves, sigma_n = 0.1 -> the left half is filtered as if the right half were holes
    n2 = np.zeros((h, w, 3), np.float32)
    n2[:, :w // 2, 0] = 1.0
    n2[:, w // 2:, 1] = 1.0
    cut = img.copy()
    cut[:, w // 2:] = 0.0
    a = texpost.denoise(dev(img), nrm=dev(n2), sigma=(0.5, 0.1, 0.25)).cpu().numpy()[:, :w // 2]
    b = texpost.denoise(dev(cut)).cpu().numpy()[:, :w // 2]
    e2 = rel_l2(a, b)
    print("guided identities on the device: constant guides %.3e, half planes %.3e (bound 1e-6)" % (e1, e2))
    assert e1 <= 1e-6 and e2 <= 1e-6
    assert rel_l2(a, _cpu_denoise(cut)[:, :w // 2]) <= BOUND


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_stage_writes_a_mat_ready_irt_hdr(tmp_path):
    from texir_code_amd import conf as C, datasets as D, io_formats as IO
    from texir_code_amd.trainer import exp_runner as ER
    root = str(tmp_path / "ds")
    sc = D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
    mesh_dir = os.path.join(root, "vrproc", "hdr_texture")
    irr_path, irt_path = os.path.join(mesh_dir, "0_irr_texture.hdr"), os.path.join(mesh_dir, "irt.hdr")
    conf_irt = str(tmp_path / "irt.conf")
    D.write_conf(conf_irt, root, cube_res=16, spp=(64, 16), model="irt")
    base = open(conf_irt).read()

    def run(extra, name):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(base + extra)
        ER.main(["--conf", path, "--trainstage", "IrrT", "--gpu", "0"])
        return open(irr_path, "rb").read()

    plain = run("", "plain.conf")
    assert not os.path.exists(irt_path)                          # without the keys: today's files, nothing else
    irr = IO.read_hdr(irr_path)
    assert (irr.sum(-1) == 0).any()                              # the atlas has gutters
    # pad only: irt.hdr = the same texture with the holes filled
    assert run("\ntrain{\n    irt_pad = nearest\n}\n", "pad.conf") == plain
    padded = IO.read_hdr(irt_path)
    nz = irr.sum(-1) != 0
    assert padded.shape == irr.shape and np.array_equal(padded[nz], irr[nz]) and not (padded.sum(-1) == 0).any()
    os.remove(irt_path)
    # pad + guided denoise
    assert run("\ntrain{\n    irt_pad = nearest\n    irt_denoise = guided\n}\n", "guided.conf") == plain
    irt = IO.read_hdr(irt_path)
    assert irt.shape == irr.shape and np.isfinite(irt).all() and not (irt.sum(-1) == 0).any()
    assert rel_l2(irt[nz], irr[nz]) < 0.5                         # still the same texture
    with pytest.raises(ValueError):
        run("\ntrain{\n    irt_denoise = guided\n}\n", "bad.conf")
    # Mat from the produced irt.hdr
    conf_mat = str(tmp_path / "mat.conf")
    D.write_conf(conf_mat, root, cube_res=16, spp=(64, 16), albedo_res=128, rough_res=128, epochs=1, model="mat")
    D.render_gt_views(root, C.parse_file(conf_mat), sc, 128, 128)
    from texir_code_amd.trainer.train_material import MatTrainRunner
    runner = MatTrainRunner(conf=conf_mat, exps_folder_name=str(tmp_path / "exps"), expname="t", frame_skip=1, max_niters=10, is_continue=False,
                            timestamp="latest", checkpoint="latest", gpu_index=0)
    runner.run()
    log = np.array(runner.log)
    assert log.shape[0] == 3 * 2 * 4 and np.isfinite(log).all()
