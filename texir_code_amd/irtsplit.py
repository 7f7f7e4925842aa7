"""Helpers around Scene.irt_split (include/texir_hip.h texir_irt_split): label images for the split and the linear algebra on its result.

Irradiance is linear in the radiance texture.  With E[k] the share of class k's texels in every texel's irradiance, any recolouring, dimming or
switching off of a class is a weighted sum of the E[k] -- what the reference re-traces per view and per colour (models/test_nvdiffrast.py:268-274:
every atlas texel brighter than 0.5 becomes one colour, the diffuse term is traced again at 64 spp)."""
import numpy as np

LUMA = (0.299, 0.587, 0.114)


def labels_from_radiance(tex, exposure, threshold=0.5):
    """the reference's lamp rule (models/test_nvdiffrast.py:268-270): a texel whose intensity 0.299 r + 0.587 g + 0.114 b of tex * 2^-exposure lies above
    the threshold is class 1 (a light source), every other texel class 0.  tex [H,W,3] float32 (the texture as the scene holds it) -> uint8 [H,W]"""
    t = np.asarray(tex, np.float32) * np.float32(2.0 ** -float(exposure))
    lum = np.float32(LUMA[0]) * t[..., 0] + np.float32(LUMA[1]) * t[..., 1] + np.float32(LUMA[2]) * t[..., 2]
    return (lum > np.float32(threshold)).astype(np.uint8)


def labels_from_seg(seg, groups):
    """seg [H,W] integer class image, groups {segmentation id: split class}, e.g. {45: 1, 46: 2}; everything else is class 0 -> uint8 [H,W]"""
    seg = np.asarray(seg)
    out = np.zeros(seg.shape, np.uint8)
    for sid, k in groups.items():
        if not 0 <= int(k) <= 255:
            raise ValueError("split class %r of segmentation id %r is not a uint8" % (k, sid))
        out[seg == sid] = k
    return out


def _xp(a):
    try:
        import torch
        if torch.is_tensor(a):
            return torch
    except ImportError:
        pass
    return np


def _colour(c, like):
    if _xp(like) is np:
        return np.asarray(c, like.dtype).reshape(-1)
    import torch
    return torch.as_tensor(c, dtype=like.dtype, device=like.device).reshape(-1)


def combine(E, colours):
    """sum_k colours[k] * E[k]: E [K,...,3], colours [K] scalars or [K,3] -> [...,3]; the irradiance under the texture tex * colours[label]"""
    if len(colours) != E.shape[0]:
        raise ValueError("%d colours for %d classes" % (len(colours), E.shape[0]))
    out = None
    for k in range(E.shape[0]):
        term = E[k] * _colour(colours[k], E)
        out = term if out is None else out + term
    return out


def replace_constant(E, F, k, colour):
    """sum_{j != k} E[j] + colour * F[k]: class k's texels become ONE colour (F from a unit=True call: the reference's "lamp texels become one
    colour"), every other class keeps its radiance"""
    if E.shape != F.shape:
        raise ValueError("E %r and F %r differ in shape" % (tuple(E.shape), tuple(F.shape)))
    if not 0 <= k < E.shape[0]:
        raise ValueError("class %d of %d" % (k, E.shape[0]))
    out = F[k] * _colour(colour, F)
    for j in range(E.shape[0]):
        if j != k:
            out = out + E[j]
    return out
