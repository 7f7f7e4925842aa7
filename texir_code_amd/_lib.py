"""ctypes loader for libtexir_hip.so (C-ABI declared in include/texir_hip.h).

There is no CPU fallback: if the shared library is missing or a call fails, a TexirError is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TEXIR_HIP_LIB") or os.path.join(_HERE, "libtexir_hip.so")   # (override: A/B builds of the kernels)
_LIB = None

class TexirError(RuntimeError):
    pass


def build():
    """compile libtexir_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc")])
    return LIB_PATH


def signatures():
    """every TEXIR_API function of include/texir_hip.h, in the header's order: name -> argtypes, or (restype, argtypes) where the function does not
    return an int32 status (tests/test_cabi.py holds the table against the header)"""
    vp, i32, i64, f32, text = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_char_p
    bake = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp]
    lights = [vp, vp, vp, vp, vp, i64, i64, vp, i32, i32, f32, vp, vp, vp]
    spec_lights = [vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, i32, i32, f32, f32, vp, vp, vp]
    mesh = [vp, i32, vp, vp, i32, C.c_uint32]      # occluders, Q, inst_obj, inst_world_to_obj, J, flags: before F / R
    return {
        "texir_last_error": (text, []),
        "texir_version": [],
        "texir_reload_env": [],
        "texir_env_switch": [text, C.POINTER(i32)],
        "texir_scene_create": [vp, i32, vp, i32, vp, vp, i32, i32, i32, C.POINTER(vp)],
        "texir_scene_destroy": [vp],
        "texir_scene_set_texture": [vp, vp, i32, i32, i32, vp],
        "texir_scene_texture_layout": [vp, vp],
        "texir_scene_bounds": [vp, vp],
        "texir_texel_pack": [vp, i64, vp, vp],
        "texir_texel_unpack": [vp, i64, vp],
        "texir_scene_info": [vp, vp],
        "texir_scene_tune": [vp, vp, vp, vp, vp, i64, i32, i32, vp],
        "texir_scene_scheduler": [vp, vp],
        "texir_scene_prefetch": [vp, i32, i32, vp],
        "texir_trace_shade": [vp, vp, vp, i64, f32, vp, vp, vp, vp, vp],
        "texir_trace_occluded": [vp, vp, vp, i64, f32, f32, vp, vp, vp],
        "texir_generate_dir": [vp, vp, vp, i64, i32, i32, vp, vp],
        "texir_irt_generate": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, vp, vp],
        "texir_scene_reserve_scratch": [vp, i64, i32],
        "texir_irt_split_workspace_bytes": (i64, [i64, i32, i32]),
        "texir_irt_split": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, i32, i32, vp, vp, i64, vp],
        "texir_irt_multi_workspace_bytes": (i64, [i64, i32, i32]),
        "texir_irt_multi": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, i32, vp, vp, i64, vp],
        "texir_irt_shadow_workspace_bytes": (i64, [i64, i32, i32]),
        "texir_irt_shadow": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, i32, vp, i32, vp, vp, vp, i64, vp],
        "texir_irt_shadow_mesh_workspace_bytes": (i64, [i64, i32, i32]),
        "texir_irt_shadow_mesh": [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, C.c_uint32, vp, i64, vp],
        "texir_irt_kernel_name": [vp, i64, i32, text, i32],
        "texir_irt_kernel_variant": [vp, i64, i32, i32, i32, text, i32],
        "texir_spec_forward": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, f32, i32, vp, vp, vp],
        "texir_spec_forward_train": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, f32, i32, vp, vp, vp, vp],
        "texir_spec_backward_ws": [vp, vp, vp, vp, i64, i32, vp, vp, vp],
        "texir_spec_backward": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, f32, vp, vp, vp],
        "texir_diffuse_irradiance": [vp, vp, vp, vp, i64, i32, i32, vp, vp],
        "texir_loss_workspace_bytes": (i64, [i64, i32, i32]),
        "texir_loss_forward": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp],
        "texir_scene_set_corner_normals": [vp, vp],
        "texir_gbuffer_cast": [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
        "texir_mip_levels": [i32, i32, i32],
        "texir_mip_elems": (i64, [i32, i32, i32, i32]),
        "texir_mip_build": [vp, vp, i32, i32, i32, i32, i32, vp],
        "texir_tex_fetch_forward": [vp, vp, i32, i32, i32, i32, vp, vp, i32, i64, vp, vp],
        "texir_tex_fetch_backward": [vp, vp, i32, i32, i32, i32, vp, vp, i32, i64, vp, vp],
        "texir_tex_fetch_backward_deferred": [vp, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp],
        "texir_tex_taps": [i32, i32, i32, i32, vp, vp, i32, i64, vp, vp, vp],
        "texir_tex_gather_backward": [vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp],
        "texir_adam_step": [vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, f32, f32, vp],
        "texir_adam_step_tex": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, i32, f32, f32, vp],
        "texir_adam_tick": [vp, vp, i32, C.c_uint64, vp],
        "texir_adam_step_dev": [vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, f32, vp],
        "texir_adam_step_tex_dev": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, f32, f32, f32, f32, f32, vp],
        "texir_batch_last_error": (text, []),
        "texir_tex_fetch_forward_batch": [vp, i32, vp],
        "texir_tex_gather_backward_batch": [vp, i32, vp],
        "texir_grad_add_masked": [vp, vp, vp, i64, i32, vp],
        "texir_adam_step_tex_dev_batch": [vp, i32, vp],
        "texir_texture_pad_workspace_bytes": (i64, [i32, i32]),
        "texir_texture_pad": [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp],
        "texir_texture_denoise": [vp, i32, i32, vp, vp, i32, f32, f32, f32, vp, vp, vp],
        "texir_texel_gbuffer_workspace_bytes": [vp, i32, i32, C.POINTER(i64)],
        "texir_texel_gbuffer": [vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp],
        "texir_atlas_bake": bake,
        "texir_atlas_bake_any": bake,
        "texir_atlas_gather": [vp, vp, vp, i64, i64, vp, i32, i32, i32, i32, vp, vp],
        "texir_atlas_fill_workspace_bytes": (i64, [i64, i64]),
        "texir_atlas_fill_cell": (f32, [vp, i64, f32]),
        "texir_atlas_fill": [vp, vp, i64, vp, i64, vp, i64, vp, f32, f32, f32, vp, vp, vp, vp, vp],
        "texir_irt_lights": lights,
        "texir_irt_lights_any": lights,
        "texir_spec_lights": spec_lights,
        "texir_spec_lights_any": spec_lights,
        "texir_irt_lights_mesh": lights[:-3] + mesh + lights[-3:],
        "texir_spec_lights_mesh": spec_lights[:-3] + mesh + spec_lights[-3:],
        "texir_spec_shadow": [vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, f32, vp, i32, vp, i32, vp, vp, i32, vp, i32, C.c_uint32, vp, vp, vp],
        "texir_gbuffer_cast_mesh": [vp, vp, i32, i32] + mesh + [vp, vp, vp, vp, vp, vp, vp, vp],
        "texir_png_unfilter": [vp, i32, i32, i32, vp],
        "texir_hdr_decode_scanlines": (i64, [vp, i64, i32, i32, vp]),
        "texir_rgbe_encode": [vp, i64, vp],
        "texir_hdr_encode_rle": (i64, [vp, i32, i32, vp, i64]),
        "texir_rgbe_decode": [vp, i64, vp],
        "texir_obj_parse": [vp, i64, C.POINTER(vp), vp],
        "texir_obj_take": [vp, vp, vp, vp, vp, vp, vp],
    }


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TexirError("libtexir_hip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "-- there is no CPU fallback" % LIB_PATH)
        # Device pointers and streams come from PyTorch-ROCm, so the kernels must be launched through the SAME HIP
        # runtime instance torch uses: torch bundles its own libamdhip64.so (soname libamdhip64.so.7, the soname our
        # library needs), so load torch -- and pin its runtime -- before dlopen()ing ours.
        import torch
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            C.CDLL(tl, mode=C.RTLD_GLOBAL)
        L = C.CDLL(LIB_PATH)
        for name, entry in signatures().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = entry if isinstance(entry, tuple) else (C.c_int32, entry)
        _LIB = L
    return _LIB


class TexFetchJob(C.Structure):
    """texir_tex_fetch_job (include/texir_hip.h)"""
    _fields_ = [("tex", C.c_void_p), ("mips_rest", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("levels", C.c_int32),
                ("build_from", C.c_int32), ("filter_mode", C.c_int32), ("uv", C.c_void_p), ("uv_da", C.c_void_p), ("P", C.c_int64), ("out", C.c_void_p)]


class TexGatherJob(C.Structure):
    """texir_tex_gather_job"""
    _fields_ = [("d_tex", C.c_void_p), ("grad_rest", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("levels", C.c_int32),
                ("seg_key", C.c_void_p), ("seg_start", C.c_void_p), ("seg_count", C.c_void_p), ("n_seg", C.c_int32), ("pix", C.c_void_p),
                ("weights", C.c_void_p), ("d_out", C.c_void_p), ("filter_mode", C.c_int32), ("defer_last_fold", C.c_int32), ("rest_mask", C.c_void_p), ("d_out2", C.c_void_p)]


class AdamTexJob(C.Structure):
    """texir_adam_tex_job"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("grad_mask", C.c_void_p), ("grad_level1", C.c_void_p), ("level1_mask", C.c_void_p),
                ("grad_level2", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("mip_level1", C.c_void_p),
                ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("hyper", C.c_void_p),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("clamp_lo", C.c_float), ("clamp_hi", C.c_float)]


MAX_BATCH = 4


def addr(t):
    """data pointer of a contiguous tensor as a plain int (ctypes Structure fields), or None"""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def batch_call(name, jobs):
    """one batched launch sequence (texir_*_batch) over a list of job structures"""
    L = lib()
    arr = (type(jobs[0]) * len(jobs))(*jobs)
    rc = getattr(L, name)(arr, len(jobs), stream_ptr())
    if rc != 0:
        raise TexirError("libtexir_hip: %s (code %d)" % (L.texir_batch_last_error().decode(), rc))


def env_switch(name):
    """the library's own (load-time or last texir_reload_env) reading of a TEXIR_* switch"""
    v = C.c_int32()
    check(lib().texir_env_switch(name.encode(), C.byref(v)))
    return int(v.value)


def reload_env():
    """re-read the library's TEXIR_* switches (parsed once at load, csrc/env.h) after os.environ was changed"""
    if _LIB is not None:
        _LIB.texir_reload_env()


def check(rc):
    if rc != 0:
        raise TexirError("libtexir_hip: %s (code %d)" % (lib().texir_last_error().decode(), rc))


def ptr(t):
    """device/host pointer of a contiguous tensor / ndarray, or None"""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        assert t.is_contiguous(), "tensor must be contiguous"
        return C.c_void_p(t.data_ptr())
    return t.ctypes.data_as(C.c_void_p)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
