"""Inserted emitters for Scene.irt_lights (include/texir_hip.h texir_irt_lights): light records, their file form and the linear algebra on the result.

Irradiance is linear in emitted radiance.  With F[k] the per-texel geometry-and-visibility factor of light k (traced once, Scene.irt_lights), the
irradiance with the lights switched on at radiance colours[k] is E + sum_k colours[k] * F[k] -- what the "moving" half of the reference's relighting demo
(tools/relighting_varying.py) leaves to an external renderer.

Bounce light.  Under light k texel y throws back the radiance albedo(y) / pi * colours[k] * F[k](y); its irradiance elsewhere is the IrT estimator on that
radiance as the texture (Scene.irt_multi, K textures in one traced pass): bounce_textures / bounce / add_indirect, and add_view(G=...) for a view.

The body's shadow.  A lamp is a body too: Scene.irt_shadow gives, per set of bodies, the part `lost` of the captured irradiance E that arrived along rays
a body of the set now intercepts; add(E, F, colours, lost=) and add_view(..., lost=) take it away, floored at zero, before the new light is added.
Computed: the direct light of the new emitters, its bounces off the scene's DIFFUSE albedo, and the shadow the emitters' bodies cast on the captured
DIFFUSE light; with Scene.spec_shadow and add_view(lost_spec=) also the shadow bodies and inserted mesh objects cast in the SPECULAR term of the captured
light, as one union.  Not computed: bodies shadowing each other's direct light or the bounce, the body drawn in a view, and any specular bounce."""
import json

import numpy as np

MAX_LIGHTS = 8
QUAD, SPHERE = 0.0, 1.0
PI32 = float(np.float32(np.pi))              # pi as the kernels have it


def _vec3(v, what):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError("%s must be three finite numbers, got %r" % (what, v))
    return a


def quad(o, a, b):
    """a parallelogram with corner o and edges a, b, emitting towards a x b (one-sided: a two-sided panel is two records) -> float32 [16]"""
    o, a, b = _vec3(o, "o"), _vec3(a, "a"), _vec3(b, "b")
    if not np.cross(a, b).any():
        raise ValueError("quad with zero area: a = %r, b = %r" % (a.tolist(), b.tolist()))
    r = np.zeros(16, np.float32)
    r[0], r[1:4], r[4:7], r[7:10] = QUAD, o, a, b
    return r


def sphere(c, r):
    """a sphere of radius r around c, emitting outwards -> float32 [16]"""
    c, rad = _vec3(c, "c"), float(r)
    if not (np.isfinite(rad) and rad > 0):
        raise ValueError("sphere radius must be finite and > 0, got %r" % (r,))
    out = np.zeros(16, np.float32)
    out[0], out[1:4], out[4] = SPHERE, c, rad
    return out


def pack(records):
    """a list of quad() / sphere() records (or a [K,16] array) -> float32 [K,16], K <= 8: what Scene.irt_lights takes"""
    recs = [np.asarray(r, np.float32).reshape(-1) for r in records]
    if len(recs) > MAX_LIGHTS:
        raise ValueError("%d lights, at most %d per call (the factors of further calls add)" % (len(recs), MAX_LIGHTS))
    for i, r in enumerate(recs):
        if r.shape != (16,):
            raise ValueError("light %d: a record is 16 floats, got %r" % (i, r.shape))
        if r[0] not in (QUAD, SPHERE):
            raise ValueError("light %d: unknown kind %r" % (i, float(r[0])))
    return np.ascontiguousarray(np.stack(recs) if recs else np.zeros((0, 16)), np.float32)


def load(path):
    """{"lights": [{"kind": "quad", "o": [..], "a": [..], "b": [..], "colour": [..]}, {"kind": "sphere", "c": [..], "r": .., "colour": [..]}]}
    -> (records float32 [K,16], colours float32 [K,3]; a light without a colour gets 1, 1, 1)"""
    with open(path) as fh:
        doc = json.load(fh)
    if not isinstance(doc, dict) or not isinstance(doc.get("lights"), list):
        raise ValueError('%s: expected {"lights": [...]}' % path)
    recs, cols = [], []
    for i, l in enumerate(doc["lights"]):
        try:
            kind = l["kind"]
            if kind == "quad":
                recs.append(quad(l["o"], l["a"], l["b"]))
            elif kind == "sphere":
                recs.append(sphere(l["c"], l["r"]))
            else:
                raise ValueError("unknown kind %r" % (kind,))
            col = np.asarray(l.get("colour", (1.0, 1.0, 1.0)), np.float64).reshape(-1)
            if col.shape == (1,):
                col = np.repeat(col, 3)
            if col.shape != (3,) or not np.isfinite(col).all():
                raise ValueError("colour must be one or three finite numbers, got %r" % (l.get("colour"),))
        except (KeyError, TypeError) as e:
            raise ValueError("%s: light %d: missing or malformed field (%s)" % (path, i, e))
        except ValueError as e:
            raise ValueError("%s: light %d: %s" % (path, i, e))
        cols.append(col)
    return pack(recs), np.asarray(cols, np.float32).reshape(-1, 3)


def _colour(c, like):
    if isinstance(like, np.ndarray):
        return np.asarray(c, like.dtype).reshape(-1)
    import torch
    return torch.as_tensor(c, dtype=like.dtype, device=like.device).reshape(-1)


def _floor0(x):
    if isinstance(x, np.ndarray):
        return np.maximum(x, x.dtype.type(0))
    return x.clamp(min=0)


def add(E, F, colours, lost=None):
    """E + sum_k colours[k] * F[k][..., None]: E [...,3] the irradiance without the lights, F [K,...] their factors, colours [K] scalars or [K,3] emitted
    radiances -> [...,3].  lost [...,3]: what the lights' bodies take from E (Scene.irt_shadow, the set of the lights switched in) -- the sum then starts
    from max(E - lost, 0); lost=None: the bits it returned without the keyword.  numpy or torch; the terms are added in ascending k"""
    if len(colours) != F.shape[0]:
        raise ValueError("%d colours for %d lights" % (len(colours), F.shape[0]))
    if tuple(F.shape[1:]) != tuple(E.shape[:-1]) or E.shape[-1] != 3:
        raise ValueError("E %r and F %r do not match ([...,3] and [K,...])" % (tuple(E.shape), tuple(F.shape)))
    out = E
    if lost is not None:
        if tuple(lost.shape) != tuple(E.shape):
            raise ValueError("lost %r must be shaped as E %r" % (tuple(lost.shape), tuple(E.shape)))
        out = _floor0(E - lost)
    for k in range(F.shape[0]):
        out = out + F[k][..., None] * _colour(colours[k], E)
    return out


def add_view(rgb, albedo, F, R, colours, G=None, lost=None, irr=None, lost_spec=None):
    """a view relit by inserted emitters: rgb + sum_k colours[k] * (albedo / pi * F[k] + R[k]).  rgb, albedo [...,3]; F [K,...] the lights' irradiance
    factors at the view's pixels (Scene.irt_lights), R [K,...] their specular response factors (Scene.spec_lights); colours [K] scalars or [K,3] -> [...,3].
    G: the lights' bounce irradiance at the view's pixels (bounce), [K,...,3] per unit colour -- then colours[k] * (albedo / pi * G[k]) is added too, after
    the direct terms -- or [...,3], already weighted and summed over the lights (add_indirect on zeros): albedo / pi * G is added.  With G=None the result
    is what it was without the keyword, bit for bit.  lost [...,3]: what the lights' bodies take from the captured irradiance at the view's pixels
    (Scene.irt_shadow), with irr [...,3] the captured irradiance rgb's diffuse term albedo / pi * irr was made of: the diffuse term becomes
    albedo / pi * max(irr - lost, 0), i.e. albedo / pi * (irr - max(irr - lost, 0)) is taken from rgb before anything is added.  Without irr the
    floor acts on the whole pixel: max(rgb - albedo / pi * lost, 0).  lost=None: the bits of the call without the keyword.  lost_spec [...,3]: what the
    bodies and the inserted objects take from the SPECULAR term of the captured light at the view's pixels (Scene.spec_shadow): max(rgb - lost_spec, 0) is
    taken first, before the diffuse correction and before anything is added.  lost_spec=None: the bits of the call without the keyword.  numpy or torch;
    the terms are added in ascending k"""
    if len(colours) != F.shape[0] or tuple(R.shape) != tuple(F.shape):
        raise ValueError("%d colours, F %r, R %r: one colour per light and R shaped as F" % (len(colours), tuple(F.shape), tuple(R.shape)))
    if tuple(F.shape[1:]) != tuple(rgb.shape[:-1]) or rgb.shape[-1] != 3 or tuple(albedo.shape) != tuple(rgb.shape):
        raise ValueError("rgb %r, albedo %r and F %r do not match ([...,3], [...,3] and [K,...])" % (tuple(rgb.shape), tuple(albedo.shape), tuple(F.shape)))
    if lost_spec is not None:
        if tuple(lost_spec.shape) != tuple(rgb.shape):
            raise ValueError("lost_spec %r must be shaped as rgb %r" % (tuple(lost_spec.shape), tuple(rgb.shape)))
        rgb = _floor0(rgb - lost_spec)
    out = rgb
    pi = _colour([PI32], rgb)                     # (an array, not a scalar: a torch division by a Python scalar multiplies by its reciprocal)
    if lost is not None:
        if tuple(lost.shape) != tuple(rgb.shape) or (irr is not None and tuple(irr.shape) != tuple(rgb.shape)):
            raise ValueError("lost (and irr) must be shaped as rgb %r" % (tuple(rgb.shape),))
        if irr is None:
            out = _floor0(rgb - albedo / pi * lost)
        else:
            out = rgb - albedo / pi * (irr - _floor0(irr - lost))
    for k in range(F.shape[0]):
        out = out + (albedo / pi * F[k][..., None] + R[k][..., None]) * _colour(colours[k], rgb)
    if G is not None:
        if tuple(G.shape) == tuple(rgb.shape):
            out = out + albedo / pi * G
        elif tuple(G.shape) == (F.shape[0],) + tuple(rgb.shape):
            for k in range(F.shape[0]):
                out = out + (albedo / pi * G[k]) * _colour(colours[k], rgb)
        else:
            raise ValueError("G %r must be [K,...,3] = %r or the summed [...,3]" % (tuple(G.shape), (F.shape[0],) + tuple(rgb.shape)))
    return out


def add_indirect(E, G, colours):
    """E + sum_k colours[k] * G[k]: E [...,3] an irradiance (add's result), G [K,...,3] the lights' bounce irradiance per unit colour (bounce), colours [K]
    scalars or [K,3] -> [...,3].  numpy or torch; the terms are added in ascending k"""
    if len(colours) != G.shape[0]:
        raise ValueError("%d colours for %d lights" % (len(colours), G.shape[0]))
    if tuple(G.shape[1:]) != tuple(E.shape) or E.shape[-1] != 3:
        raise ValueError("E %r and G %r do not match ([...,3] and [K,...,3])" % (tuple(E.shape), tuple(G.shape)))
    out = E
    for k in range(G.shape[0]):
        out = out + G[k] * _colour(colours[k], E)
    return out


def _resized(img, hw):
    """[n,H,W,c] -> [n,Ht,Wt,c]: nothing when the size is hw already, else bilinear (align_corners=False), antialiased when an axis shrinks"""
    import torch
    H, W = int(img.shape[1]), int(img.shape[2])
    if (H, W) == tuple(hw):
        return img
    x = torch.nn.functional.interpolate(img.permute(0, 3, 1, 2), size=tuple(hw), mode="bilinear", align_corners=False, antialias=hw[0] < H or hw[1] < W)
    return x.permute(0, 2, 3, 1)


def bounce_textures(albedo, F, tex_hw, src=None):
    """the radiance the scene throws back under K lights of unit colour, as textures for Scene.irt_multi: albedo [Ha,Wa,3] and F [K,H,W] (irt_lights'
    factors) or [K,H,W,3] (a bounce's irradiance), both in FILE orientation -> float32 [K,Ht,Wt,3] = (albedo / pi) * F[k] in the SCENE's orientation
    (rows reversed, as models.py holds hdr_texture and labels), tex_hw = (Ht, Wt) the scene's texture size.  An image of another size is resized
    first (bilinear, align_corners=False, antialiased when it shrinks); one of that size is used as it is, unrounded.  src: int [Ht,Wt], file
    orientation, the nearest-covered-texel map texpost.pad_texture(cover, return_src=True) gives for the COVERAGE image (-1: no source): an uncovered
    texel takes its source's radiance, so that bilinear footprints at chart edges do not darken; a covered texel keeps its own value, F = 0 (a shadow)
    included.  src=None: nothing is filled.  numpy or torch in, torch out (on F's device)"""
    import torch
    Ht, Wt = int(tex_hw[0]), int(tex_hw[1])
    F = torch.as_tensor(F)
    dev = F.device
    F = F.to(torch.float32)
    albedo = torch.as_tensor(albedo).to(device=dev, dtype=torch.float32)
    if albedo.ndim != 3 or albedo.shape[-1] != 3:
        raise ValueError("albedo must be [Ha,Wa,3], got %r" % (tuple(albedo.shape),))
    if F.ndim == 3:
        F = F[..., None]
    if F.ndim != 4 or F.shape[-1] not in (1, 3):
        raise ValueError("F must be [K,H,W] or [K,H,W,3], got %r" % (tuple(F.shape),))
    if Ht < 1 or Wt < 1:
        raise ValueError("tex_hw must be positive, got %r" % (tuple(tex_hw),))
    pi = torch.tensor([PI32], dtype=torch.float32, device=dev)            # (a tensor: see add_view)
    rad = (_resized(albedo[None], (Ht, Wt))[0] / pi) * _resized(F, (Ht, Wt))
    if src is not None:
        s = torch.as_tensor(src).to(dev)
        if tuple(s.shape) != (Ht, Wt):
            raise ValueError("src must be [%d,%d] (the coverage map of the texture), got %r" % (Ht, Wt, tuple(s.shape)))
        s = s.reshape(-1).long()
        flat = rad.reshape(rad.shape[0], Ht * Wt, 3)
        rad = torch.where((s >= 0)[None, :, None], flat[:, s.clamp(min=0)], flat).reshape(-1, Ht, Wt, 3)
    return torch.flip(rad, dims=(1,)).contiguous()


def bounce(scene, pos, nrm, shift, albedo, F, n_samples, bounces=1, texel_ids=None, hw=None, src=None):
    """the bounce irradiance of K inserted lights of unit colour at the listed points: G [K,Nt,3] = sum over b = 1..bounces of G_b, added in ascending b,
    G_1 = scene.irt_multi(bounce_textures(albedo, F)), G_b = scene.irt_multi(bounce_textures(albedo, G_{b-1})).  pos / nrm / shift [Nt,...] are the texel
    list of an hw = (H, W) atlas in file orientation (default: F's own H, W), so that G_{b-1} is an image again; albedo, F, src: as bounce_textures takes
    them.  Diffuse bounces of the NEW light only (see the module's docstring)"""
    import torch
    bounces = int(bounces)
    if bounces < 1:
        raise ValueError("bounces must be >= 1, got %d" % bounces)
    F = torch.as_tensor(F)
    if F.ndim not in (3, 4):
        raise ValueError("F must be [K,H,W] or [K,H,W,3], got %r" % (tuple(F.shape),))
    K = int(F.shape[0])
    H, W = (int(v) for v in (hw if hw is not None else F.shape[1:3]))
    Nt = int(pos.shape[0]) if pos.ndim == 2 else int(np.prod(pos.shape[:-1]))
    if bounces > 1 and Nt != H * W:
        raise ValueError("%d points are not the texels of a %d x %d atlas: a second bounce needs the whole atlas" % (Nt, H, W))
    tex_hw = tuple(int(v) for v in scene.tex_shape[:2])
    total, last = None, F
    for b in range(1, bounces + 1):
        last = scene.irt_multi(pos, nrm, shift, n_samples, bounce_textures(albedo, last, tex_hw, src), texel_ids=texel_ids)
        total = last if total is None else total + last
        if b < bounces:
            last = last.reshape(K, H, W, 3)
    return total
