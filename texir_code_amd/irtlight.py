"""Inserted emitters for Scene.irt_lights (include/texir_hip.h texir_irt_lights): light records, their file form and the linear algebra on the result.

Irradiance is linear in emitted radiance.  With F[k] the per-texel geometry-and-visibility factor of light k (traced once, Scene.irt_lights), the
irradiance with the lights switched on at radiance colours[k] is E + sum_k colours[k] * F[k] -- what the "moving" half of the reference's relighting demo
(tools/relighting_varying.py) leaves to an external renderer.  Direct light only."""
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


def add(E, F, colours):
    """E + sum_k colours[k] * F[k][..., None]: E [...,3] the irradiance without the lights, F [K,...] their factors, colours [K] scalars or [K,3] emitted
    radiances -> [...,3].  numpy or torch; the terms are added in ascending k"""
    if len(colours) != F.shape[0]:
        raise ValueError("%d colours for %d lights" % (len(colours), F.shape[0]))
    if tuple(F.shape[1:]) != tuple(E.shape[:-1]) or E.shape[-1] != 3:
        raise ValueError("E %r and F %r do not match ([...,3] and [K,...])" % (tuple(E.shape), tuple(F.shape)))
    out = E
    for k in range(F.shape[0]):
        out = out + F[k][..., None] * _colour(colours[k], E)
    return out


def add_view(rgb, albedo, F, R, colours):
    """a view relit by inserted emitters: rgb + sum_k colours[k] * (albedo / pi * F[k] + R[k]).  rgb, albedo [...,3]; F [K,...] the lights' irradiance
    factors at the view's pixels (Scene.irt_lights), R [K,...] their specular response factors (Scene.spec_lights); colours [K] scalars or [K,3] -> [...,3].
    numpy or torch; the terms are added in ascending k"""
    if len(colours) != F.shape[0] or tuple(R.shape) != tuple(F.shape):
        raise ValueError("%d colours, F %r, R %r: one colour per light and R shaped as F" % (len(colours), tuple(F.shape), tuple(R.shape)))
    if tuple(F.shape[1:]) != tuple(rgb.shape[:-1]) or rgb.shape[-1] != 3 or tuple(albedo.shape) != tuple(rgb.shape):
        raise ValueError("rgb %r, albedo %r and F %r do not match ([...,3], [...,3] and [K,...])" % (tuple(rgb.shape), tuple(albedo.shape), tuple(F.shape)))
    out = rgb
    pi = _colour([PI32], rgb)                     # (an array, not a scalar: a torch division by a Python scalar multiplies by its reciprocal)
    for k in range(F.shape[0]):
        out = out + (albedo / pi * F[k][..., None] + R[k][..., None]) * _colour(colours[k], rgb)
    return out
