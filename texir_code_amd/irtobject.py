"""Inserted mesh objects for Scene.irt_shadow_mesh (include/texir_hip.h texir_irt_shadow_mesh): the conf / json form of `train.irt_objects`, poses, the sets
the IrT stage asks for and the linear algebra of `object-irt`.

    train.irt_objects = none | [ { "obj": <path of an .obj>, "pose": <4 x 4 (or 3 x 4) object-to-world, rows> } , ... ]
                             | [ { "obj": ..., "pose": { "translate": [x, y, z], "rotate_deg": [rx, ry, rz], "scale": s | [sx, sy, sz] } }, ... ]
                             | <path of a json file that holds such a list, bare or under the key "objects">
`rotate_deg` are rotations about the world's x, then y, then z axis, applied after the scale and before the translation: M = T Rz Ry Rx S.  A missing pose
is the identity.  At most 8 objects; two entries may name one file (it is loaded and built once).
With the key the IrT stage writes, beside 0_irr_texture.hdr, 0_irr_texture_object<k>_shadow.hdr -- the part of the irradiance that arrived along rays object
k now intercepts -- and for K > 1 0_irr_texture_objects_shadow.hdr, the same for all objects together (a union, not the sum).  `object-irt` subtracts one of
them from the base: max(E - lost, 0).  The objects' shadow on the inserted emitters' light F and R is Scene.irt_lights / spec_lights(occluders=...):
train.irt_light_objects in the stage, test.objects in the evaluation model.  The objects drawn in a view and lit by the lamps: gbuffer.cast_gbuffer(occluders=...), test.draw_objects
with test.object_materials (materials() below) in the evaluation model.  Not computed: the bounce G's own rays (they ignore the objects)."""
import json
import math
import os

import numpy as np

MAX_OBJECTS = 8
KEY = "train.irt_objects"


def pose_matrix(pose):
    """a 4 x 4 / 3 x 4 nested list, or {"translate", "rotate_deg", "scale"} (each optional), or None -> object-to-world [3,4] float64; ValueError names
    what is wrong"""
    if pose is None:
        return np.eye(3, 4)
    if isinstance(pose, dict):
        unknown = sorted(set(pose) - {"translate", "rotate_deg", "scale"})
        if unknown:
            raise ValueError("%s: a pose has the keys translate, rotate_deg and scale, not %s" % (KEY, ", ".join(map(str, unknown))))
        try:
            t = np.asarray(pose.get("translate", [0, 0, 0]), np.float64).reshape(-1)
            r = np.asarray(pose.get("rotate_deg", [0, 0, 0]), np.float64).reshape(-1)
            s = np.asarray(pose.get("scale", 1.0), np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("%s: translate, rotate_deg and scale must be numbers, got %r" % (KEY, pose))
        if t.shape != (3,) or r.shape != (3,) or s.shape not in ((1,), (3,)):
            raise ValueError("%s: translate and rotate_deg take three numbers, scale one or three, got %r" % (KEY, pose))
        cx, cy, cz = (math.cos(math.radians(a)) for a in r)
        sx, sy, sz = (math.sin(math.radians(a)) for a in r)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        M = np.concatenate([(Rz @ Ry @ Rx) * (np.repeat(s, 3) if s.shape == (1,) else s), t[:, None]], 1)
    else:
        try:
            M = np.asarray(pose, np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: a pose is a 4 x 4 matrix or {translate, rotate_deg, scale}, got %r" % (KEY, pose))
        if M.shape == (4, 4):
            if not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
                raise ValueError("%s: the last row of a 4 x 4 pose must be 0 0 0 1, got %r" % (KEY, M[3].tolist()))
            M = M[:3]
        if M.shape != (3, 4):
            raise ValueError("%s: a pose is a 4 x 4 (or 3 x 4) matrix or {translate, rotate_deg, scale}, got shape %r" % (KEY, M.shape))
    if not np.isfinite(M).all():
        raise ValueError("%s: a pose has a non-finite entry" % KEY)
    return M


def parse(spec, base_dir=None):
    """the value of train.irt_objects -> None (none) | [(path, pose [3,4] float64), ...]; relative .obj paths of a json FILE are taken from its directory.
    ValueError / FileNotFoundError name the key"""
    if spec is None or (isinstance(spec, str) and spec.strip().lower() == "none"):
        return None
    if isinstance(spec, str):
        path = spec
        if not os.path.exists(path):
            raise FileNotFoundError("%s = %s: no such file" % (KEY, path))
        with open(path) as f:
            try:
                spec = json.load(f)
            except ValueError as e:
                raise ValueError("%s = %s: not json (%s)" % (KEY, path, e))
        base_dir = os.path.dirname(os.path.abspath(path))
        if isinstance(spec, dict):
            spec = spec.get("objects")
    if not isinstance(spec, (list, tuple)) or not spec:
        raise ValueError("%s must be none, a list of {obj, pose} or a json file of one, got %r" % (KEY, spec))
    if len(spec) > MAX_OBJECTS:
        raise ValueError("%s names %d objects: at most %d" % (KEY, len(spec), MAX_OBJECTS))
    out = []
    for k, e in enumerate(spec):
        if not isinstance(e, dict) or "obj" not in e or set(e) - {"obj", "pose"}:
            raise ValueError("%s: entry %d must be {obj, pose}, got %r" % (KEY, k, e))
        path = str(e["obj"])
        if base_dir is not None and not os.path.isabs(path):
            path = os.path.join(base_dir, path)
        out.append((path, pose_matrix(e.get("pose"))))
    return out


MATERIALS_KEY = "test.object_materials"
DEFAULT_ALBEDO, DEFAULT_ROUGHNESS = 0.5, 0.5
ROUGHNESS_RANGE = (0.01, 0.8)             # the range the trainer clamps a roughness texture to


def materials(spec, n_objects):
    """the value of test.object_materials -> (albedo [K,3], roughness [K]) float32, one row per object of test.objects:
        none | [ { "albedo": g | [r, g, b], "roughness": r }, ... ] | <path of a json file that holds such a list, bare or under the key "materials">
    Either key may be missing: albedo 0.5, roughness 0.5.  ValueError names the key: a list of another length than the objects', an albedo that is not
    finite or negative, a roughness outside [0.01, 0.8]"""
    K = int(n_objects)
    albedo, rough = np.full((K, 3), DEFAULT_ALBEDO, np.float32), np.full((K,), DEFAULT_ROUGHNESS, np.float32)
    if spec is None or (isinstance(spec, str) and spec.strip().lower() == "none"):
        return albedo, rough
    if isinstance(spec, str):
        path = spec
        if not os.path.exists(path):
            raise FileNotFoundError("%s = %s: no such file" % (MATERIALS_KEY, path))
        with open(path) as f:
            try:
                spec = json.load(f)
            except ValueError as e:
                raise ValueError("%s = %s: not json (%s)" % (MATERIALS_KEY, path, e))
        if isinstance(spec, dict):
            spec = spec.get("materials")
    if not isinstance(spec, (list, tuple)):
        raise ValueError("%s must be none, a list of {albedo, roughness} or a json file of one, got %r" % (MATERIALS_KEY, spec))
    if len(spec) != K:
        raise ValueError("%s has %d entries for %d objects: one entry per object" % (MATERIALS_KEY, len(spec), K))
    for k, e in enumerate(spec):
        if not isinstance(e, dict) or set(e) - {"albedo", "roughness"}:
            raise ValueError("%s: entry %d must be {albedo, roughness}, got %r" % (MATERIALS_KEY, k, e))
        try:
            a = np.asarray(e.get("albedo", DEFAULT_ALBEDO), np.float64).reshape(-1)
            r = float(e.get("roughness", DEFAULT_ROUGHNESS))
        except (TypeError, ValueError):
            raise ValueError("%s: entry %d: albedo is a number or [r, g, b], roughness a number, got %r" % (MATERIALS_KEY, k, e))
        if isinstance(e.get("roughness"), bool) or a.shape not in ((1,), (3,)):
            raise ValueError("%s: entry %d: albedo is a number or [r, g, b], roughness a number, got %r" % (MATERIALS_KEY, k, e))
        if not np.isfinite(a).all() or (a < 0).any():
            raise ValueError("%s: entry %d: albedo must be finite and >= 0, got %r" % (MATERIALS_KEY, k, e.get("albedo")))
        if not ROUGHNESS_RANGE[0] <= r <= ROUGHNESS_RANGE[1]:
            raise ValueError("%s: entry %d: roughness must be in [%g, %g], got %r" % ((MATERIALS_KEY, k) + ROUGHNESS_RANGE + (e.get("roughness"),)))
        albedo[k], rough[k] = a, r
    return albedo, rough


def samples_setting(conf, default_samples):
    """train.irt_object_samples (default: the stage's own sample count -- the shadow is a part of THAT estimate) -> int >= 1"""
    s = conf.get("train.irt_object_samples", default_samples)
    try:
        if isinstance(s, bool) or int(s) != float(s) or int(s) < 1:
            raise ValueError
        return int(s)
    except (TypeError, ValueError):
        raise ValueError("train.irt_object_samples must be an integer >= 1, got %r" % (s,))


def shadow_sets(K):
    """the sets the stage asks Scene.irt_shadow_mesh for, as calls of at most 8 sets: one per object and, for K > 1, the union of all"""
    singles = [[k] for k in range(K)]
    union = [list(range(K))] if K > 1 else []
    return [singles + union] if K + len(union) <= 8 else [singles, union]


def load(objects, device=None):
    """[(path, pose)] -> (occluders: one Scene.occluder per distinct file, instances [K], poses [K,3,4])"""
    from . import io_formats as IO
    from .scene import Scene
    handles, index, inst = [], {}, []
    for path, _ in objects:
        key = os.path.abspath(path)
        if key not in index:
            if not os.path.exists(path):
                raise FileNotFoundError("%s: no such file %s" % (KEY, path))
            obj = IO.load_obj(path, cache=False)
            index[key] = len(handles)
            handles.append(Scene.occluder(obj["vertices"], obj["indices"], device=device))
        inst.append(index[key])
    return handles, inst, np.stack([p for _, p in objects])


def shadow_file(directory, objects=None):
    """the file object-irt subtracts for the named objects (None: all) -> path.  One object: its own file; every object of the directory: the union file
    (the single file when there is one object); any other subset, or a missing file: FileNotFoundError naming the file and the conf key"""
    import re
    have = sorted(int(m.group(1)) for m in (re.fullmatch(r"0_irr_texture_object(\d+)_shadow\.hdr", n) for n in os.listdir(directory)) if m)
    named = have if objects is None else sorted(set(int(k) for k in objects))
    if not named:
        raise FileNotFoundError("no 0_irr_texture_object<k>_shadow.hdr in %s: run the IrT stage with %s = <list of {obj, pose}>" % (directory, KEY))
    if len(named) == 1:
        f = os.path.join(directory, "0_irr_texture_object%d_shadow.hdr" % named[0])
    elif named == have:
        f = os.path.join(directory, "0_irr_texture_objects_shadow.hdr")
    else:
        raise FileNotFoundError("the objects %s: the stage writes the shadow of one object (0_irr_texture_object<k>_shadow.hdr) and of all %d together "
                                "(0_irr_texture_objects_shadow.hdr), no other subset: name one object or all (%s)" % (named, len(have), KEY))
    if not os.path.exists(f):
        raise FileNotFoundError("object-irt needs %s: run the IrT stage with %s = <list of {obj, pose}>" % (f, KEY))
    return f


def object_irt(directory, objects=None, base=None):
    """0_irr_texture_objects.hdr = max(base - lost, 0) for the named objects (None: all) -> the path written; existing files are not overwritten"""
    from . import io_formats as IO, irtlight
    dst = os.path.join(directory, "0_irr_texture_objects.hdr")
    if os.path.exists(dst):
        raise FileExistsError("%s exists: not overwritten" % dst)
    base = os.path.join(directory, "0_irr_texture.hdr") if base is None else base
    if not os.path.exists(base):
        raise FileNotFoundError("no %s: run the IrT stage first, or name the base with --base" % base)
    f = shadow_file(directory, objects)
    E, lost = np.asarray(IO.read_hdr(base), np.float32), np.asarray(IO.read_hdr(f), np.float32)
    if lost.shape != E.shape:
        raise ValueError("%s is %r, the base %s is %r" % (f, lost.shape, base, E.shape))
    out = irtlight.add(E, np.zeros((0,) + E.shape[:2], np.float32), [], lost=lost)
    IO.write_hdr(dst, np.ascontiguousarray(out, np.float32))
    return dst
