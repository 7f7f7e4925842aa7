"""Cube-map G-buffers by primary-ray casting (replaces dr.rasterize + dr.interpolate, models/mat_nvdiffrast.py:119-128)."""
import numpy as np
import torch

from . import _lib


def set_corner_normals(scene, corner_normals):
    """corner_normals [3T,3] = normals[indices] (pyredner.load_obj order, tracer_o3d_irt.py:61)"""
    a = np.ascontiguousarray(corner_normals, np.float32).reshape(-1, 3)
    if a.shape[0] != 3 * scene.n_tris:
        raise ValueError("corner_normals must be [3T,3]")
    _lib.check(_lib.lib().texir_scene_set_corner_normals(scene.h, _lib.ptr(a)))


NORMAL_MODES = {"geometric": 0, "shading": 1}


def raster_texel_gbuffer(scene, H, W, normal="geometric", offset=1e-2, want_ids=False):
    """The texel G-buffer of an H x W atlas as a uv-space rasterisation of the scene's triangles (texir_texel_gbuffer, csrc/texraster.hip; replaces
    tracer_o3d_irt.py:99-142 and needs no index texture).  Returns device tensors in FILE orientation (what texel_gbuffer.npz holds):
    pos [H,W,3] = surface point + offset * normal, nrm [H,W,3]; uncovered texels are all-zero seams.  normal = "geometric" (face normal) or
    "shading" (interpolated corner normals of set_corner_normals, not renormalised).  want_ids adds prim_id [H,W] int64 (-1: seam) and
    bary [H,W,2] (weights of the caller's corners 1 and 2).  Launches on the current stream without synchronising it."""
    if normal not in NORMAL_MODES:
        raise ValueError("raster_texel_gbuffer: normal must be geometric or shading, got %r" % (normal,))
    H, W = int(H), int(W)
    dev = scene.device
    L = _lib.lib()
    import ctypes as C
    nb = C.c_int64()
    _lib.check(L.texir_texel_gbuffer_workspace_bytes(scene.h, H, W, C.byref(nb)))
    ws = torch.empty(max(1, int(nb.value)), device=dev, dtype=torch.uint8)
    pos = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    nrm = torch.empty((H, W, 3), device=dev, dtype=torch.float32)
    ids = torch.empty((H, W), device=dev, dtype=torch.int32) if want_ids else None
    bary = torch.empty((H, W, 2), device=dev, dtype=torch.float32) if want_ids else None
    _lib.check(L.texir_texel_gbuffer(scene.h, H, W, NORMAL_MODES[normal], float(offset), _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(ids), _lib.ptr(bary),
                                     _lib.ptr(ws), _lib.stream_ptr()))
    if want_ids:
        return pos, nrm, ids.long(), bary          # (0xFFFFFFFF reads as int32 -1)
    return pos, nrm


def cast_gbuffer(scene, mvp, cube_res, flip_v=False):
    """mvp [6,4,4] (row-vector convention, datasets/dataset.py:464-465) -> dict of [6,c,c,k] tensors:
    position, normal, mask, uv (texc), uv_da (texd), tri_id"""
    dev = scene.device
    m = np.ascontiguousarray(mvp.detach().to("cpu", torch.float32).numpy().reshape(6, 4, 4))
    c = int(cube_res)
    P = 6 * c * c
    f = lambda k: torch.empty((P, k), device=dev, dtype=torch.float32)
    pos, nrm, mask, uv, uvda = f(3), f(3), f(1), f(2), f(4)
    tri = torch.empty((P,), device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().texir_gbuffer_cast(scene.h, _lib.ptr(m), c, 1 if flip_v else 0, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(mask),
                                             _lib.ptr(uv), _lib.ptr(uvda), _lib.ptr(tri), _lib.stream_ptr()))
    r = lambda t, k: t.reshape(6, c, c, k)
    return {"position": r(pos, 3), "normal": r(nrm, 3), "mask": r(mask, 1), "uv": r(uv, 2), "uv_da": r(uvda, 4), "tri_id": tri.reshape(6, c, c)}
