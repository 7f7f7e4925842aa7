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


def cast_gbuffer(scene, mvp, cube_res, flip_v=False, occluders=None, instances=None, poses=None, prefilter=True):
    """mvp [6,4,4] (row-vector convention, datasets/dataset.py:464-465) -> dict of [6,c,c,k] tensors:
    position, normal, mask, uv (texc), uv_da (texd), tri_id.
    occluders, instances, poses: inserted mesh objects DRAWN IN THE VIEW (texir_gbuffer_cast_mesh), with the meaning and the host / device forms of
    Scene.irt_shadow_mesh: Q <= 8 handles of Scene.occluder, J <= 8 indices into them, poses [J,3,4] OBJECT-TO-WORLD on the host (inverted in float64) or a
    [J,12] WORLD-TO-OBJECT float32 DEVICE tensor used in place (a recorded graph replays with whatever it holds then).  The dict then also has inst_id
    [6,c,c] int32: -1 where the pixel shows the room or nothing (those pixels hold the bits of the call without occluders), else the instance; an instance
    pixel has the world-space position and normal of the object's surface, tri_id = the object's own triangle + 1, mask = 1, uv = uv_da = 0.
    prefilter=False: every lane walks every valid instance (the same bits, slower).  occluders=None is the call as it always was."""
    c = int(cube_res)
    if occluders is None:
        if instances is not None or poses is not None:
            raise ValueError("cast_gbuffer: instances and poses need occluders")
    else:
        if not 1 <= c <= 16384:
            raise ValueError("cast_gbuffer: cube_res must be in 1..16384, got %d" % c)
        occluders = list(occluders)
        inst_list = [] if instances is None else [int(k) for k in np.asarray(instances).reshape(-1)]
        if len(occluders) > 8 or len(inst_list) > 8:
            raise ValueError("cast_gbuffer: a call takes at most 8 occluders and 8 instances, got %d and %d" % (len(occluders), len(inst_list)))
        if any(not 0 <= k < len(occluders) for k in inst_list):
            raise ValueError("cast_gbuffer: instances %r name no occluder (Q = %d)" % (inst_list, len(occluders)))
        if tuple(mvp.shape) != (6, 4, 4):
            raise ValueError("cast_gbuffer: mvp must be [6,4,4], got %r" % (tuple(mvp.shape),))
    dev = scene.device
    m = np.ascontiguousarray(mvp.detach().to("cpu", torch.float32).numpy().reshape(6, 4, 4))
    P = 6 * c * c
    f = lambda k: torch.empty((P, k), device=dev, dtype=torch.float32)
    pos, nrm, mask, uv, uvda = f(3), f(3), f(1), f(2), f(4)
    tri = torch.empty((P,), device=dev, dtype=torch.int32)
    r = lambda t, k: t.reshape(6, c, c, k)
    if occluders is None:
        _lib.check(_lib.lib().texir_gbuffer_cast(scene.h, _lib.ptr(m), c, 1 if flip_v else 0, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(mask),
                                                 _lib.ptr(uv), _lib.ptr(uvda), _lib.ptr(tri), _lib.stream_ptr()))
        return {"position": r(pos, 3), "normal": r(nrm, 3), "mask": r(mask, 1), "uv": r(uv, 2), "uv_da": r(uvda, 4), "tri_id": tri.reshape(6, c, c)}
    import ctypes as C
    from .scene import mesh_instances
    _, handles, Q, inst, w2o, J = mesh_instances(dev, occluders, instances, poses)
    iid = torch.empty((P,), device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().texir_gbuffer_cast_mesh(scene.h, _lib.ptr(m), c, 1 if flip_v else 0, C.cast(handles, C.c_void_p) if Q else None, Q,
                                                  _lib.ptr(inst) if J else None, _lib.ptr(w2o) if J else None, J, 0 if prefilter else 1, _lib.ptr(pos),
                                                  _lib.ptr(nrm), _lib.ptr(mask), _lib.ptr(uv), _lib.ptr(uvda), _lib.ptr(tri), _lib.ptr(iid), _lib.stream_ptr()))
    return {"position": r(pos, 3), "normal": r(nrm, 3), "mask": r(mask, 1), "uv": r(uv, 2), "uv_da": r(uvda, 4), "tri_id": tri.reshape(6, c, c),
            "inst_id": iid.reshape(6, c, c)}
