"""The asset step between the two stages on the device (tools/padding_texture.py:49-87): pad the zero texels of the irradiance texture from their
nearest non-zero texel and denoise it -- texir_texture_pad / texir_texture_denoise of include/texir_hip.h (csrc/texpost.hip).

Device tensors in, device tensors out; failures raise TexirError; there is no CPU fallback here (tools.padding_texture / tools.denoise_atrous are
the CPU restatements the tests compare against).

    pad_texture(img, mode)          mode = "nearest": every hole takes the value of a non-hole texel at minimal Euclidean distance;
                                    mode = "reference": the reference's accident bit for bit -- its F.grid_sample(mode="nearest", align_corners=False)
                                    reads source index i at rint(i - 0.5), one texel too low for every odd row / column, often a hole again: about a
                                    third of the gutter texels stay black (tools.py's docstring has the figures).
    denoise(img, nrm, pos, ...)     edge-avoiding a-trous filter, colour-only or guided by the texel G-buffers.
"""
import numpy as np
import torch

from . import _lib

MODES = ("nearest", "reference")


def reference_index_map(n):
    """int32 [n]: the source index F.grid_sample(mode='nearest', align_corners=False) reads when tools.padding_texture asks for index i of an axis of length
    n (-1: outside, i.e. zero padding), as a float32 statement of its arithmetic: u = i / n * 2 - 1 (padding_texture's normalisation), x = ((u + 1) * n - 1) / 2
    (grid_sample's un-normalisation), j = rint(x), half to even."""
    f = np.float32
    i = np.arange(n, dtype=np.float32)
    u = i / f(n) * f(2.0) - f(1.0)
    x = ((u + f(1.0)) * f(n) - f(1.0)) / f(2.0)
    j = np.rint(x).astype(np.int64)
    j[(j < 0) | (j >= n)] = -1
    return j.astype(np.int32)


def _dev_f32(t, what, last=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.TexirError("texpost: %s must be a device tensor" % what)
    if t.dim() != 3 or (last is not None and t.shape[-1] != last):
        raise _lib.TexirError("texpost: %s must be [H,W,%s], got %s" % (what, last or "C", tuple(t.shape)))
    return t.detach().to(torch.float32).contiguous()


def pad_texture(img, mode="nearest", return_src=False):
    """img [H,W,C] (device, C in 1..4) -> padded copy; with return_src also src [H,W] int32: the flat index of the texel each texel took its value from
    (itself for a non-hole, -1 everywhere when the image has no non-hole texel) -- the same sources pad companion images: comp.reshape(-1, c)[src]."""
    if mode not in MODES:
        raise ValueError("texpost.pad_texture: mode must be nearest or reference, got %r" % (mode,))
    x = _dev_f32(img, "img")
    H, W, C = x.shape
    L = _lib.lib()
    out = torch.empty_like(x)
    src = torch.empty((H, W), device=x.device, dtype=torch.int32) if return_src else None
    ws = torch.empty(max(1, int(L.texir_texture_pad_workspace_bytes(H, W))), device=x.device, dtype=torch.uint8)
    rm = cm = None
    if mode == "reference":
        rm = torch.from_numpy(reference_index_map(H)).to(x.device)
        cm = torch.from_numpy(reference_index_map(W)).to(x.device)
    _lib.check(L.texir_texture_pad(_lib.ptr(x), H, W, C, _lib.ptr(rm), _lib.ptr(cm), _lib.ptr(out), _lib.ptr(src), _lib.ptr(ws), _lib.stream_ptr()))
    return (out, src) if return_src else out


def gather_src(comp, src):
    """pad a companion image [H,W,c] (a guide) with the sources pad_texture returned: one torch gather"""
    H, W, c = comp.shape
    flat = comp.reshape(H * W, c)
    s = src.reshape(-1).long()
    return torch.where((s >= 0)[:, None], flat[s.clamp(min=0)], flat).reshape(H, W, c)


def denoise(img, nrm=None, pos=None, iterations=3, sigma=(0.5, 0.3, 0.25)):
    """img [H,W,3] (device) -> denoised [H,W,3]; nrm / pos [H,W,3] optional guides; sigma = (sigma_c, sigma_n, sigma_p), a guide sigma of 0 switches its
    term off."""
    x = _dev_f32(img, "img", 3)
    H, W, _ = x.shape
    sc, sn, sp = (float(s) for s in sigma)
    g = []
    for name, t in (("nrm", nrm), ("pos", pos)):
        if t is not None:
            t = _dev_f32(t, name, 3)
            if t.shape != x.shape:
                raise _lib.TexirError("texpost.denoise: %s is %s, the image %s" % (name, tuple(t.shape), tuple(x.shape)))
        g.append(t)
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().texir_texture_denoise(_lib.ptr(x), H, W, _lib.ptr(g[0]), _lib.ptr(g[1]), int(iterations), sc, sn, sp, _lib.ptr(tmp), _lib.ptr(out),
                                                _lib.stream_ptr()))
    return out
