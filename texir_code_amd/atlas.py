"""The radiance atlas (hdr_texture.hdr) and the index texture (0.png) of a mesh from calibrated HDR panoramas, on the device.

Every stage starts from those two files; the reference produces neither (its private capture pipeline writes 0.png, tools/trans_hdr_tex.py:16-61 only gathers
the panoramas' pixels through its codes).  texir_atlas_bake (csrc/texbake.hip; include/texir_hip.h states the rule) picks per texel the view that faces it,
sees it un-occluded and maximises cosine over squared distance, and the panorama pixel utils/Pano2Cube.py:57-82 reads for the texel's direction.

    python -m texir_code_amd.tools bake-atlas <root> <res|HxW> [--out DIR] [--cos-min X] [--normal geometric|shading] [--seg]
                                              [--fill] [--fill-dist D] [--fill-cos C]

--fill completes what the bake leaves: texir_atlas_fill (csrc/texfill.hip) names, per covered texel no panorama sees, the nearest OBSERVED texel in world
space whose normal agrees (fill_atlas), and dilate_gutters gives the texels outside every chart their uv-nearest covered texel.

THE CAMERA FRAME.  A final_extrinsics.txt matrix E is camera-to-world with columns (right, column 1, front, position).  cameras.cube_mvps' front face uses
inverse(E) as it is and puts face row 0 at ndc y = -1, i.e. at NEGATIVE camera y; Pano2Cube's front face has row 0 at sy = +1 and measures
azimuth = atan2(x, z), elevation = asin(y) (x right, y up, z front).  So Pano2Cube's frame is diag(1, -1, 1) inverse(E): camera_matrices folds the sign of y
into W.  The other five faces follow from the same frame (cube_mvps' column table and Pano2Cube's rotations agree face by face); tests pin it.
"""
import math
import os

import numpy as np
import torch

from . import _lib

CODE_MAX = 50000


def camera_matrices(extrinsics):
    """c2w matrices [K,4,4] (final_extrinsics.txt) -> (W [K,3,4] float32 world -> Pano2Cube camera frame, cam_pos [K,3] float32)"""
    E = np.asarray(extrinsics, np.float64).reshape(-1, 4, 4)
    inv = np.linalg.inv(E)
    S = np.diag([1.0, -1.0, 1.0])
    W = np.einsum("ij,kjl->kil", S, inv[:, 0:3, :])
    return torch.from_numpy(np.ascontiguousarray(W, np.float32)), torch.from_numpy(np.ascontiguousarray(E[:, 0:3, 3], np.float32))


def pano_xy(W, points):
    """float64 statement of the pixel rule before the floor: W [3,4], points [...,3] -> (x, y) continuous panorama coordinates in units of w and h
    (multiply by w, h), i.e. x = (az / pi + 1) / 2, y = (1 - el / (pi / 2)) / 2"""
    W = torch.as_tensor(W, dtype=torch.float64)
    p = torch.as_tensor(points, dtype=torch.float64)
    t = p @ W[:, 0:3].T + W[:, 3]
    az = torch.atan2(t[..., 0], t[..., 2])
    el = torch.asin((t[..., 1] / t.norm(dim=-1)).clamp(-1.0, 1.0))
    return (az / math.pi + 1.0) / 2.0, (1.0 - el / (math.pi / 2.0)) / 2.0


def pano_pixel(W, points, h, w):
    """float64 statement of the pixel rule: W [3,4] (one view of camera_matrices), points [...,3] -> (row, col) int64 of an h x w panorama: the pixel
    Pano2Cube's grid_sample(nearest, align_corners=False) reads for the point's direction"""
    x, y = pano_xy(W, points)
    col = torch.floor(x * w).clamp(0, w - 1).long()
    row = torch.floor(y * h).clamp(0, h - 1).long()
    return row, col


def _f32(t, dev, shape):
    return torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(*shape).contiguous()


def bake_atlas(scene, pos, nrm, W, cam_pos, panos, valid=None, cos_min=0.1, texel_ids=None, out=None, stats=False, query="closest"):
    """texir_atlas_bake.  pos (already offset), nrm [..,3]; W [K,3,4], cam_pos [K,3] (camera_matrices); panos [K,h,w,3] float32; valid [K,h,w] uint8 or None;
    texel_ids: int32 list of the texels to decide (None: all; pass dist_util.morton_order's order) -> view [Nt] int32 (-1: no view), pix [Nt,2] int32
    (row, col), rgb [Nt,3] float32.  Unlisted texels keep what `out` = (view, pix, rgb) held (fresh buffers: view -1, zeros).  stats=True adds a
    [4] int64 tensor (pairs facing, pairs traced, pairs visible, texels assigned).  query: 'closest' | 'any' (texir_atlas_bake_any: the segment test as an
    occlusion query, the same bits).  Launches on the current stream, no synchronisation."""
    from .scene import check_query
    call = "texir_atlas_bake_any" if check_query(query, "bake_atlas: query") else "texir_atlas_bake"
    dev = scene.device
    pos, nrm = _f32(pos, dev, (-1, 3)), _f32(nrm, dev, (-1, 3))
    Nt = pos.shape[0]
    panos = torch.as_tensor(panos).to(device=dev, dtype=torch.float32).contiguous()
    if panos.ndim != 4 or panos.shape[3] != 3:
        raise ValueError("bake_atlas: panos must be [K,h,w,3]")
    K, h, w = int(panos.shape[0]), int(panos.shape[1]), int(panos.shape[2])
    W, cam_pos = _f32(W, dev, (-1, 12)), _f32(cam_pos, dev, (-1, 3))
    if W.shape[0] != K or cam_pos.shape[0] != K or nrm.shape[0] != Nt:
        raise ValueError("bake_atlas: %d panoramas, %d matrices, %d positions; %d pos, %d nrm" % (K, W.shape[0], cam_pos.shape[0], Nt, nrm.shape[0]))
    if valid is not None:
        valid = torch.as_tensor(valid).to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(valid.shape) != (K, h, w):
            raise ValueError("bake_atlas: valid must be [K,h,w]")
    if out is None:
        out = (torch.full((Nt,), -1, device=dev, dtype=torch.int32), torch.zeros((Nt, 2), device=dev, dtype=torch.int32),
               torch.zeros((Nt, 3), device=dev, dtype=torch.float32))
    view, pix, rgb = out
    ids, n_ids = None, 0
    if texel_ids is not None:
        ids = texel_ids.to(device=dev, dtype=torch.int32).contiguous()
        n_ids = ids.numel()
    st = torch.zeros(4, device=dev, dtype=torch.int64) if stats else None
    if Nt > 0 and not (texel_ids is not None and n_ids == 0):          # (an empty list must not reach the library: NULL means all texels)
        _lib.check(getattr(_lib.lib(), call)(scene.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(ids), n_ids, Nt, _lib.ptr(W), _lib.ptr(cam_pos), _lib.ptr(panos),
                                             _lib.ptr(valid), K, h, w, float(cos_min), _lib.ptr(view), _lib.ptr(pix), _lib.ptr(rgb), _lib.ptr(st), _lib.stream_ptr()))
    return (view, pix, rgb, st) if stats else (view, pix, rgb)


def gather_atlas(view, pix, images, texel_ids=None, out=None):
    """texir_atlas_gather: images [K,h,w,C] (C = 1..4; any dtype, gathered as float32) through (view [Nt], pix [Nt,2]) -> [Nt,C] float32, zeros where
    view < 0: the device form of the repack*Texture gathers of tools/trans_hdr_tex.py"""
    dev = view.device
    img = torch.as_tensor(images).to(device=dev, dtype=torch.float32)
    if img.ndim == 3:
        img = img[..., None]
    img = img.contiguous()
    K, h, w, C = (int(v) for v in img.shape)
    view = view.to(torch.int32).reshape(-1).contiguous()
    Nt = view.shape[0]
    pix = pix.to(torch.int32).reshape(Nt, 2).contiguous()
    if out is None:
        out = torch.zeros((Nt, C), device=dev, dtype=torch.float32)
    ids, n_ids = None, 0
    if texel_ids is not None:
        ids = texel_ids.to(device=dev, dtype=torch.int32).contiguous()
        n_ids = ids.numel()
    if Nt > 0 and not (texel_ids is not None and n_ids == 0):
        _lib.check(_lib.lib().texir_atlas_gather(_lib.ptr(view), _lib.ptr(pix), _lib.ptr(ids), n_ids, Nt, _lib.ptr(img), K, h, w, C, _lib.ptr(out), _lib.stream_ptr()))
    return out


def scene_bounds(vertices, offset=1e-2):
    """host vertices [V,3] -> float32 [6] = (min, max) grown by the G-buffer's offset: the box fill_atlas bins its sources over"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    return np.concatenate([v.min(0) - offset, v.max(0) + offset]).astype(np.float32)


def _fill_bounds(bounds, pos, lists):
    if bounds is not None:
        b = np.ascontiguousarray(np.asarray(bounds, np.float32).reshape(6))
        if not np.isfinite(b).all() or (b[3:] < b[:3]).any():
            raise ValueError("fill_atlas: bounds must be six finite numbers (min xyz, max xyz), got %s" % b.tolist())
        return b
    ids = torch.cat([l.reshape(-1).long() for l in lists])
    ids = ids[(ids >= 0) & (ids < pos.shape[0])]
    if ids.numel() == 0:
        return np.array([0, 0, 0, 1, 1, 1], np.float32)
    p = pos[ids]
    p = torch.where(torch.isfinite(p), p, torch.zeros_like(p))
    return torch.cat([p.min(0).values, p.max(0).values]).cpu().numpy().astype(np.float32)


def fill_cell(bounds, n_src, cell=0.0):
    """the grid cell edge texir_atlas_fill searches with for these arguments (cell = 0: the library's choice)"""
    b = np.ascontiguousarray(np.asarray(bounds, np.float32).reshape(6))
    return float(_lib.lib().texir_atlas_fill_cell(_lib.ptr(b), int(n_src), float(cell)))


def fill_atlas(pos, nrm, source_ids, hole_ids, cos_fill=0.5, max_dist=0.5, bounds=None, out=None, stats=False, dist2=False, cell=0.0):
    """texir_atlas_fill.  pos (already offset), nrm [..,3] device float32 (the G-buffer bake_atlas took); source_ids: the observed texels, hole_ids: the
    texels to decide (int32 lists; pass the holes in dist_util.morton_order's order) -> src [Nt] int32: per listed hole the nearest source in world space
    within max_dist whose normal agrees (cosine >= cos_fill), lowest id on an exact tie, or -1.  Unlisted texels keep what `out` = src or (src, dist2) held
    (a fresh src is -1 everywhere, a fresh dist2 zero).  dist2=True adds the float32 squared distances [Nt], stats=True a [2] int64 tensor (holes decided,
    holes filled).  bounds: six host numbers (scene_bounds: the scene's vertices grown by the offset) that steer speed only; None takes the listed
    positions' own box from the device, which costs one device-to-host copy -- pass bounds to launch on the current stream with no synchronisation.
    cell: the grid's cell edge, 0 = the library chooses (fill_cell reports it)."""
    if not torch.is_tensor(pos) or not pos.is_cuda:
        raise _lib.TexirError("fill_atlas: pos must be a device tensor")
    dev = pos.device
    pos, nrm = _f32(pos, dev, (-1, 3)), _f32(nrm, dev, (-1, 3))
    Nt = pos.shape[0]
    if nrm.shape[0] != Nt:
        raise ValueError("fill_atlas: %d pos, %d nrm" % (Nt, nrm.shape[0]))
    if not (0.0 <= float(cos_fill) <= 1.0) or not float(max_dist) > 0.0:
        raise ValueError("fill_atlas: cos_fill must be in [0, 1] and max_dist > 0 (got %r, %r)" % (cos_fill, max_dist))
    sid = torch.as_tensor(source_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    hid = torch.as_tensor(hole_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    b = _fill_bounds(bounds, pos, (sid, hid))
    src, d2 = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
    if src is None:
        src = torch.full((Nt,), -1, device=dev, dtype=torch.int32)
    if dist2 and d2 is None:
        d2 = torch.zeros((Nt,), device=dev, dtype=torch.float32)
    st = torch.zeros(2, device=dev, dtype=torch.int64) if stats else None
    L = _lib.lib()
    if hid.numel() > 0:
        ws = torch.empty(max(16, int(L.texir_atlas_fill_workspace_bytes(sid.numel(), hid.numel()))), device=dev, dtype=torch.uint8)
        _lib.check(L.texir_atlas_fill(_lib.ptr(pos), _lib.ptr(nrm), Nt, _lib.ptr(sid) if sid.numel() else None, sid.numel(), _lib.ptr(hid), hid.numel(),
                                      _lib.ptr(b), float(cos_fill), float(max_dist), float(cell), _lib.ptr(src), _lib.ptr(d2), _lib.ptr(st), _lib.ptr(ws),
                                      _lib.stream_ptr()))
    res = (src,) + ((d2,) if dist2 else ()) + ((st,) if stats else ())
    return res if len(res) > 1 else src


def gutter_targets(covered, src):
    """the index logic of dilate_gutters on host or device arrays: covered [H,W] bool, src [H,W] = the pad's source index per texel -> (flat ids of the
    texels that change, flat ids they read): the UNCOVERED texels whose source is a covered texel; covered texels never change"""
    xp = torch if torch.is_tensor(covered) else np
    c = covered.reshape(-1) != 0
    s = src.reshape(-1)
    if xp is torch:
        s = s.long()
        ok = ~c & (s >= 0)
        ok = ok & c[s.clamp(min=0)]
        t = torch.nonzero(ok)[:, 0]
    else:
        s = s.astype(np.int64)
        ok = ~c & (s >= 0)
        ok = ok & c[np.clip(s, 0, None)]
        t = np.nonzero(ok)[0]
    return t, s[t]


def dilate_gutters(image, covered):
    """image [H,W,C] (device), covered [H,W] bool -> a copy in which every UNCOVERED texel holds the value of the nearest covered texel in uv space
    (texir_texture_pad on a one-channel coverage image, then a gather of `image` through its sources); covered texels are never touched, those left black
    on purpose included.  With no covered texel at all the copy equals the image."""
    from . import texpost
    H, W = covered.shape
    cov = covered.to(device=image.device).reshape(H, W)
    _, src = texpost.pad_texture(cov.to(torch.float32)[..., None].contiguous(), mode="nearest", return_src=True)
    t, s = gutter_targets(cov, src)
    out = image.clone()
    flat = out.reshape(H * W, -1)
    flat[t] = image.reshape(H * W, -1)[s]
    return out


def index_codes(view, pix, h, w):
    """(view [..], pix [..,2]) -> uint16 [..,3] = (row code, col code, view id): the code of a pixel is round((i + 0.5) / n * 50000) clamped to [1, 50000]
    (what datasets.write_index_texture_from_panoramas stores; tools/trans_hdr_tex.py:50-53 decodes it back to i); texels without a view are all-zero,
    the reference's seam"""
    view = np.asarray(view.cpu() if torch.is_tensor(view) else view).astype(np.int64)
    pix = np.asarray(pix.cpu() if torch.is_tensor(pix) else pix).astype(np.int64)
    if view.size and view.max() > 65535:
        raise ValueError("index_codes: view id %d does not fit 16 bits" % int(view.max()))
    rc = np.clip(np.rint((pix[..., 0] + 0.5) / h * CODE_MAX), 1, CODE_MAX)
    cc = np.clip(np.rint((pix[..., 1] + 0.5) / w * CODE_MAX), 1, CODE_MAX)
    codes = np.stack([rc, cc, np.maximum(view, 0)], -1).astype(np.uint16)
    codes[view < 0] = 0
    return codes


def decode_codes(codes, h, w):
    """the inverse, as tools/trans_hdr_tex.py:50-53 decodes: (row, col) = clip(int(code / 50000 * n), 0, n - 1) -> (view [..] int64 (-1: seam), pix [..,2])"""
    c = np.asarray(codes).astype(np.int64)
    seam = c.sum(-1) == 0
    row = np.clip((c[..., 0] / CODE_MAX * h).astype(np.int64), 0, h - 1)
    col = np.clip((c[..., 1] / CODE_MAX * w).astype(np.int64), 0, w - 1)
    view = np.where(seam, -1, c[..., 2])
    pix = np.stack([np.where(seam, 0, row), np.where(seam, 0, col)], -1)
    return view, pix


def pano_directions(W, h, w):
    """world-space unit directions [h,w,3] (float64) through the pixel CENTRES of one view's h x w panorama: the inverse of the pixel rule"""
    W = torch.as_tensor(W, dtype=torch.float64)
    az = ((torch.arange(w, dtype=torch.float64) + 0.5) / w * 2.0 - 1.0) * math.pi
    el = (1.0 - (torch.arange(h, dtype=torch.float64) + 0.5) / h * 2.0) * (math.pi / 2.0)
    el, az = torch.meshgrid(el, az, indexing="ij")
    d = torch.stack([torch.sin(az) * torch.cos(el), torch.sin(el), torch.cos(az) * torch.cos(el)], -1)
    return d @ torch.linalg.inv(W[:, 0:3]).T


def trace_panoramas(scene, c2w, h, w):
    """the scene's radiance as K equirectangular panoramas [K,h,w,3] (device float32) through scene.trace_shade: one ray per pixel centre from the camera
    position along the inverse of the pixel rule.  Synthetic input for tests and the timing tool."""
    W, cam = camera_matrices(c2w)
    out = []
    for k in range(W.shape[0]):
        d = pano_directions(W[k], h, w).to(torch.float32).reshape(-1, 3)
        o = cam[k].expand_as(d).contiguous()
        out.append(scene.trace_shade(o, d).reshape(h, w, 3))
    return torch.stack(out, 0)


def read_extrinsics(root):
    """<root>/info/final_extrinsics.txt -> [K,4,4] float64 (first line is a header, datasets/dataset.py:409)"""
    with open(os.path.join(root, "info", "final_extrinsics.txt"), "r") as f:
        lines = [l.replace(" \n", "\n") for l in f.readlines()]
    return np.loadtxt(lines[1:], delimiter=" ").reshape(-1, 4, 4)


def _packs_exactly(rgb):
    """every texel is three 8-bit integers times one power of two (texir_texel_pack): the condition of the scene's 4-byte texel layout"""
    a = np.ascontiguousarray(rgb.detach().cpu().numpy().reshape(-1, 3), np.float32)
    ok = np.zeros(len(a), np.uint8)
    _lib.check(_lib.lib().texir_texel_pack(_lib.ptr(a), len(a), _lib.ptr(np.zeros(len(a), np.uint32)), _lib.ptr(ok)))
    return bool(ok.all())


def bake_files(root, H, W_atlas, out_dir=None, cos_min=0.1, normal="geometric", seg=False, device=0, fill=False, fill_dist=0.5, fill_cos=0.5, query="closest"):
    """the command: mesh + extrinsics + hdr/<id>/ccm.hdr (+ the alpha of derived/<id>/panoImage_orig.jpg as the mask) -> hdr_texture.hdr, 0.png
    (+ 0_seg_gray.png) in out_dir.  Returns a dict (paths, the share of covered texels that got a view, the device arrays).
    fill=True completes the atlas before it is written: unobserved covered texels from the nearest compatible observed texel in world space (fill_atlas,
    fill_dist scene units, cosine fill_cos), then the texels outside every chart from their uv-nearest covered texel (dilate_gutters); 0.png keeps the
    observed texels' codes only; atlas_fill.npz holds the sources; the dict gains fill_src and the counts observed, filled, black (covered texels)."""
    from . import datasets, dist_util, gbuffer as GB, imgops, io_formats as IO
    from .scene import Scene
    mesh_dir = os.path.join(root, "vrproc", "hdr_texture")
    out_dir = out_dir or os.path.join(mesh_dir, "baked")
    names = ["hdr_texture.hdr", "0.png"] + (["0_seg_gray.png"] if seg else []) + (["atlas_fill.npz"] if fill else [])
    for n in names:
        if os.path.exists(os.path.join(out_dir, n)):
            raise FileExistsError("%s exists: bake-atlas does not overwrite" % os.path.join(out_dir, n))
    with open(os.path.join(root, "info", "aligned.txt"), "r") as f:
        ids = [l.strip() for l in f.readlines() if l.strip()]
    E = read_extrinsics(root)
    if E.shape[0] != len(ids):
        raise ValueError("%d ids in aligned.txt but %d extrinsics" % (len(ids), E.shape[0]))
    panos, masks = [], []
    for i in ids:
        p = IO.read_hdr(os.path.join(root, "hdr", i, "ccm.hdr"))
        if panos and p.shape != panos[0].shape:
            raise ValueError("hdr/%s/ccm.hdr is %s, the first panorama %s" % (i, p.shape, panos[0].shape))
        panos.append(p)
        pm = os.path.join(root, "derived", i, "panoImage_orig.jpg")
        if os.path.exists(pm):
            rgba = datasets._read_pano_rgba(pm)
            a = rgba[:, :, 3] if rgba.ndim == 3 and rgba.shape[2] == 4 else np.full(rgba.shape[:2], 255, np.uint8)
            masks.append(imgops.resize_nearest(np.ascontiguousarray(a), (p.shape[1], p.shape[0])))
        else:
            masks.append(None)
    h, w = panos[0].shape[:2]
    valid = None
    if any(m is not None for m in masks):
        valid = np.stack([np.full((h, w), 255, np.uint8) if m is None else (m > 0).astype(np.uint8) * 255 for m in masks], 0)
    obj = IO.load_obj(os.path.join(mesh_dir, "out1.obj"))
    scene = Scene(obj["vertices"], obj["indices"], IO.triangle_uvs_open3d(obj), np.zeros((2, 2, 3), np.float32), device=device)       # (no radiance is read)
    if normal == "shading":
        GB.set_corner_normals(scene, IO.corner_normals(obj))
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(scene, H, W_atlas, normal=normal, want_ids=True)
    covered = torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32)
    order = dist_util.morton_order(covered, W_atlas)
    Wm, cam = camera_matrices(E)
    view, pix, rgb = bake_atlas(scene, pos, nrm, Wm, cam, np.stack(panos, 0), valid, cos_min, texel_ids=order, query=query)
    os.makedirs(out_dir, exist_ok=True)
    res = {"dir": out_dir, "view": view, "pix": pix, "rgb": rgb, "covered": int(covered.numel()), "hw": (h, w), "view_count": len(ids)}
    fill_src = filled_ids = None
    if fill:
        seen = view[order.long()] >= 0
        sources, holes = order[seen].contiguous(), order[~seen].contiguous()                  # both keep the Morton order
        fill_src = fill_atlas(pos, nrm, sources, holes, fill_cos, fill_dist, bounds=scene_bounds(obj["vertices"]))
        filled_ids = holes[fill_src[holes.long()] >= 0].long()
        born = _packs_exactly(rgb)
        rgb[filled_ids] = rgb[fill_src[filled_ids].long()]                                    # the source's bits as they are
        cov = torch.zeros(H * W_atlas, dtype=torch.bool, device=rgb.device)
        cov[covered.long()] = True
        rgb = dilate_gutters(rgb.reshape(H, W_atlas, 3), cov.reshape(H, W_atlas)).reshape(-1, 3)
        # the 4-byte texel layout (Scene.texture_layout() >= 3) is chosen when every texel packs exactly; the fill only copies texels, so it stays in force
        assert not born or _packs_exactly(rgb), "the fill copies texels: an RGBE-born atlas must stay RGBE-born"
        np.savez(os.path.join(out_dir, "atlas_fill.npz"), src=fill_src.reshape(H, W_atlas).cpu().numpy())
        res.update(rgb=rgb, fill_src=fill_src, observed=int(sources.numel()), filled=int(filled_ids.numel()),
                   black=int(holes.numel() - filled_ids.numel()))
    IO.write_hdr(os.path.join(out_dir, "hdr_texture.hdr"), rgb.reshape(H, W_atlas, 3).cpu().numpy())     # file orientation, no exposure
    codes = index_codes(view, pix, h, w).reshape(H, W_atlas, 3)
    IO.write_png(os.path.join(out_dir, "0.png"), np.ascontiguousarray(codes[..., ::-1]))                  # the file stores RGB = (view id, col code, row code)
    if seg:
        segs = []
        for i in ids:
            s = IO.read_png(os.path.join(root, "derived", i, "panoImage_gray.png"))
            s = s[..., 0] if s.ndim == 3 else s
            segs.append(imgops.resize_nearest(np.ascontiguousarray(s), (w, h)))
        g = gather_atlas(view, pix, np.stack(segs, 0).astype(np.float32))
        if fill:
            g[filled_ids] = g[fill_src[filled_ids].long()]                                    # a filled texel takes its source's class; gutters stay 0
        g = g.reshape(H, W_atlas)
        IO.write_png(os.path.join(out_dir, "0_seg_gray.png"), g.cpu().numpy().astype(np.uint8))
    n_view = int((view.reshape(-1)[covered.long()] >= 0).sum().item())
    res["share"] = n_view / max(1, res["covered"])
    return res
