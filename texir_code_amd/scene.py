"""Scene handle: the MI355X replacement of the Open3D RaycastingScene + CPU radiance texture that
TracerO3d.__init__ / MaterialModel.__init__ build (models/tracer_o3d_irt.py:75-89, models/mat_nvdiffrast.py:87-101)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MODES = {"uniform": 0, "cosine": 1, "importance": 2}
QUERIES = ("closest", "any")


def check_query(query, what="query"):
    """the visibility query of the bake and the light pass: 'closest' (one closest-hit query per ray, its t compared with the far bound) | 'any' (one
    occlusion query per ray, texir_trace_occluded's traversal: the same bits) -> True for 'any'; anything else raises ValueError"""
    if query not in QUERIES:
        raise ValueError("%s must be 'closest' or 'any', got %r" % (what, query))
    return query == "any"

# hipFree is not allowed while a stream capture (hipGraph) is in progress, and a Scene may be garbage-collected at any time:
# destruction is deferred while this counter is non-zero (see defer_destroy()).
_DEFER = [0]
_PENDING = []


class defer_destroy:
    """context manager: scene handles released inside are destroyed on exit (used around hipGraph capture)"""

    def __enter__(self):
        _DEFER[0] += 1

    def __exit__(self, *a):
        _DEFER[0] -= 1
        if _DEFER[0] == 0 and _lib._LIB is not None:
            while _PENDING:
                _lib._LIB.texir_scene_destroy(_PENDING.pop())


def world_to_object(poses):
    """poses [K,3,4] (or [K,4,4] with the last row 0 0 0 1) OBJECT-TO-WORLD on the host -> [K,12] float32 WORLD-TO-OBJECT rows, the form
    texir_irt_shadow_mesh reads: inverted in float64, rounded once.  A pose that is not finite, not affine or singular (a condition number of its 3 x 3
    part above 1e12 counts) raises ValueError naming the instance"""
    if torch.is_tensor(poses):
        poses = poses.detach().cpu().numpy()
    P = np.asarray(poses, np.float64)
    if P.ndim != 3 or P.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("poses must be [K,3,4] object-to-world (or [K,4,4]), got %r" % (P.shape,))
    out = np.zeros((P.shape[0], 12), np.float32)
    for j, p in enumerate(P):
        if not np.isfinite(p).all():
            raise ValueError("pose %d has a non-finite entry" % j)
        if p.shape[0] == 4 and not np.array_equal(p[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("pose %d is not affine: its last row is %r" % (j, p[3].tolist()))
        A, t = p[:3, :3], p[:3, 3]
        if np.linalg.det(A) == 0 or not np.linalg.cond(A) < 1e12:
            raise ValueError("pose %d is singular" % j)
        Ai = np.linalg.inv(A)
        w = np.concatenate([Ai, (-Ai @ t)[:, None]], 1)
        w32 = w.astype(np.float32)
        if not np.isfinite(w32).all():
            raise ValueError("pose %d has no float32 inverse" % j)
        out[j] = w32.reshape(12)
    return out


def mesh_instances(device, occluders, instances, poses):
    """the objects of irt_shadow_mesh, irt_lights and spec_lights in the library's form: occluders: Q <= 8 handles of Scene.occluder; instances: J <= 8
    indices into them; poses: [J,3,4] OBJECT-TO-WORLD on the host (inverted in float64 and rounded once; a singular pose is a ValueError) or a [J,12]
    WORLD-TO-OBJECT float32 DEVICE tensor, used in place -> (occluders list, handles array, Q, inst int32 [J], w2o device [J,12], J)"""
    occluders = list(occluders)
    if not all(isinstance(o, Scene) for o in occluders):
        raise ValueError("occluders must be Scene handles (Scene.occluder)")
    inst = np.ascontiguousarray(np.asarray([] if instances is None else instances, np.int64).reshape(-1), np.int32)
    K, Q = int(inst.shape[0]), len(occluders)
    if torch.is_tensor(poses) and poses.is_cuda:
        if tuple(poses.shape) != (K, 12) or poses.dtype != torch.float32 or not poses.is_contiguous() or poses.device != device:
            raise ValueError("device poses must be a contiguous float32 [%d,12] world-to-object tensor on %s" % (K, device))
        w2o = poses
    else:
        w = world_to_object(poses) if K else np.zeros((0, 12), np.float32)
        if w.shape[0] != K:
            raise ValueError("%d instances, %d poses" % (K, w.shape[0]))
        w2o = torch.from_numpy(w).to(device)
    handles = (C.c_void_p * max(Q, 1))(*[o.h for o in occluders])
    return occluders, handles, Q, inst, w2o, K


def spec_shadow_sets(sets, n_bodies, n_instances):
    """the `sets` of Scene.spec_shadow as uint32 masks (texir_spec_shadow: bit k = body k, bit 8 + j = instance j): None -> one set holding every body and
    every instance; else a list whose items are an int mask (0 .. 2^32 - 1, used as it is: the library ignores bits that name nothing) or a pair
    (body indices, instance indices), each index inside its count -- anything else is a ValueError -> list of Python ints"""
    Kb, J = int(n_bodies), int(n_instances)
    if sets is None:
        return [((1 << Kb) - 1) | (((1 << J) - 1) << 8)]
    masks = []
    for m, item in enumerate(sets):
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            if not 0 <= int(item) < 1 << 32:
                raise ValueError("set %d: a mask is a uint32, got %r" % (m, item))
            masks.append(int(item))
            continue
        try:
            if isinstance(item, (str, bytes)) or any(isinstance(part, (str, bytes)) for part in item):
                raise TypeError
            body_ids, inst_ids = item
            body_ids, inst_ids = [int(k) for k in body_ids], [int(j) for j in inst_ids]
        except (TypeError, ValueError):
            raise ValueError("set %d must be an int mask or a pair (body indices, instance indices), got %r" % (m, item))
        v = 0
        for k in body_ids:
            if not 0 <= k < Kb:
                raise ValueError("set %d names body %d: the call has %d bodies" % (m, k, Kb))
            v |= 1 << k
        for j in inst_ids:
            if not 0 <= j < J:
                raise ValueError("set %d names instance %d: the call has %d instances" % (m, j, J))
            v |= 1 << (8 + j)
        masks.append(v)
    return masks


def _dev_f32(t, device):
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).contiguous()


class Scene:
    """verts [V,3], tris [T,3] (primitive id = row, Open3D order), tri_uvs [3T,2] (= np.asarray(mesh.triangle_uvs)),
    hdr_texture [Ht,Wt,3] float32 ALREADY RGB + vertically flipped + exposure-scaled (tracer_o3d_irt.py:77-81)."""

    def __init__(self, verts, tris, tri_uvs, hdr_texture, device=None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        tri_uvs = np.ascontiguousarray(tri_uvs, np.float32).reshape(-1, 2)
        hdr = np.ascontiguousarray(hdr_texture, np.float32)
        if tri_uvs.shape[0] != 3 * tris.shape[0]:
            raise ValueError("tri_uvs must be [3T,2]")
        if hdr.ndim != 3 or hdr.shape[2] != 3:
            raise ValueError("hdr_texture must be [Ht,Wt,3]")
        self.n_tris = tris.shape[0]
        self.tex_shape = hdr.shape
        h = C.c_void_p()
        _lib.check(_lib.lib().texir_scene_create(_lib.ptr(verts), verts.shape[0], _lib.ptr(tris), tris.shape[0], _lib.ptr(tri_uvs),
                                                 _lib.ptr(hdr), hdr.shape[0], hdr.shape[1], self.device.index, C.byref(h)))
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None and getattr(_lib, "_LIB", None) is not None:      # (module globals may be gone at interpreter exit)
            try:
                if _DEFER[0] > 0:
                    _PENDING.append(h)
                else:
                    _lib._LIB.texir_scene_destroy(h)
            except Exception:
                pass
            self.h = None

    def info(self):
        out = np.zeros(8, np.int64)
        _lib.check(_lib.lib().texir_scene_info(self.h, _lib.ptr(out)))
        keys = ["inner_nodes", "triangles", "max_depth", "node_bytes", "tri_bytes", "uv_bytes", "tex_bytes", "device"]
        d = dict(zip(keys, (int(x) for x in out)))
        sch = np.zeros(2, np.float64)
        _lib.check(_lib.lib().texir_scene_scheduler(self.h, _lib.ptr(sch)))
        d["sched_weight"], d["node_step_fill"] = int(sch[0]), (None if sch[1] < 0 else round(float(sch[1]), 4))
        d["tex_layout"] = self.texture_layout()
        return d

    def texture_layout(self):
        """layout of the hit shader's texture copy in force: 3 / 4 = 4-byte shared-exponent texels (the texture packs exactly: an RGBE file times a power
        of two), 2 / 1 / 0 = float32 (include/texir_hip.h texir_scene_texture_layout)"""
        out = np.zeros(1, np.int32)
        _lib.check(_lib.lib().texir_scene_texture_layout(self.h, _lib.ptr(out)))
        return int(out[0])

    def reserve_irt_scratch(self, n_ids, n_samples):
        """before RECORDING irt_generate over n_ids listed texels into a hipGraph: reserve the partial-sum scratch the recorded launch will use (a recorded
        graph must not allocate; include/texir_hip.h texir_scene_reserve_scratch).  Eager calls need nothing."""
        _lib.check(_lib.lib().texir_scene_reserve_scratch(self.h, int(n_ids), int(n_samples)))

    def irt_kernel_name(self, n_ids, n_samples):
        """the kernel form one irt_generate call over n_ids listed texels launches (the launcher's own decision)"""
        buf = C.create_string_buffer(96)
        _lib.check(_lib.lib().texir_irt_kernel_name(self.h, int(n_ids), int(n_samples), buf, 96))
        return buf.value.decode()

    def irt_kernel_variant(self, n_ids, n_samples, mode="uniform", cosine_estimator=False):
        """the instantiation of that form the call launches for this sampling mode and estimator (include/texir_hip.h texir_irt_kernel_variant)"""
        buf = C.create_string_buffer(128)
        _lib.check(_lib.lib().texir_irt_kernel_variant(self.h, int(n_ids), int(n_samples), MODES[mode], int(bool(cosine_estimator)), buf, 128))
        return buf.value.decode()

    def set_texture(self, tex):
        """tex [Ht,Wt,3] tensor (device or host) -- stage -1's temporary light-source-only texture (mat_nvdiffrast.py:141-150)"""
        if torch.is_tensor(tex) and tex.is_cuda:
            tex = tex.to(torch.float32).contiguous()
            _lib.check(_lib.lib().texir_scene_set_texture(self.h, _lib.ptr(tex), tex.shape[0], tex.shape[1], 1, _lib.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        else:
            a = np.ascontiguousarray(tex.numpy() if torch.is_tensor(tex) else tex, np.float32)
            _lib.check(_lib.lib().texir_scene_set_texture(self.h, _lib.ptr(a), a.shape[0], a.shape[1], 0, _lib.stream_ptr()))
            torch.cuda.current_stream().synchronize()

    # -- query_irf (tracer_o3d_irt.py:240-269) ----------------------------------------------------------
    def trace_shade(self, org, dir, t_min=1e-4, return_hits=False):
        org = _dev_f32(org, self.device).reshape(-1, 3)
        dir = _dev_f32(dir, self.device).reshape(-1, 3)
        R = org.shape[0]
        rad = torch.empty((R, 3), device=self.device, dtype=torch.float32)
        t = pid = uv = None
        if return_hits:
            t = torch.empty(R, device=self.device, dtype=torch.float32)
            pid = torch.empty(R, device=self.device, dtype=torch.int32)
            uv = torch.empty((R, 2), device=self.device, dtype=torch.float32)
        if R > 0:                                   # (zero rays: empty results; an empty tensor has no pointer to hand to the library)
            _lib.check(_lib.lib().texir_trace_shade(self.h, _lib.ptr(org), _lib.ptr(dir), R, float(t_min), _lib.ptr(rad), _lib.ptr(t),
                                                    _lib.ptr(pid), _lib.ptr(uv), _lib.stream_ptr()))
        return (rad, t, pid, uv) if return_hits else rad

    # -- RaycastingScene.test_occlusions, the sibling of the cast_rays above (include/texir_hip.h texir_trace_occluded) ------------
    def test_occlusions(self, org, dir, t_near=0.0, t_far=float("inf"), out=None, stats=False):
        """is anything in the way of the ray inside (t_near, t_far), t in units of |dir|?  org, dir [..., 3] (any leading shape, as trace_shade takes) ->
        bool [R], R the number of rays: True iff some triangle passes the closest-hit query's leaf test with t_near < t < t_far.  At t_near = 0 this is
        `hit & (t_hit < t_far)` of trace_shade(return_hits=True), bit for bit, from a traversal that stops at the first accepted triangle.  t_far = nan
        or <= t_near: nothing is occluded.  out: a bool or uint8 [R] device tensor to write into.  stats=True: also int64 [1] = the occluded rays"""
        org = _dev_f32(org, self.device).reshape(-1, 3)
        dir = _dev_f32(dir, self.device).reshape(-1, 3)
        R = org.shape[0]
        if dir.shape[0] != R:
            raise ValueError("test_occlusions: %d origins, %d directions" % (R, dir.shape[0]))
        if out is None:
            out = torch.zeros(R, device=self.device, dtype=torch.bool)
        elif tuple(out.shape) != (R,) or out.dtype not in (torch.bool, torch.uint8) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous bool or uint8 [%d] on %s" % (R, self.device))
        st = torch.zeros(1, device=self.device, dtype=torch.int64) if stats else None
        if R > 0:
            _lib.check(_lib.lib().texir_trace_occluded(self.h, _lib.ptr(org), _lib.ptr(dir), R, float(t_near), float(t_far), _lib.ptr(out), _lib.ptr(st),
                                                       _lib.stream_ptr()))
        return (out, st) if stats else out

    # -- TracerO3d.forward hot loop (tracer_o3d_irt.py:156-178) -------------------------------------------
    def irt_generate(self, pos, nrm, shift, n_samples, mode="uniform", texel_ids=None, out=None, stats=False):
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        if out is None:
            out = torch.zeros((Nt, 3), device=self.device, dtype=torch.float32)
        ids = None
        n_ids = 0
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n_ids = ids.numel()
        st = torch.zeros(32, device=self.device, dtype=torch.int64) if stats else None         # [0:8] counters (include/texir_hip.h); [8:26] cycle probe of a TEXIR_CHAIN_PROBE build
        if Nt == 0 or (texel_ids is not None and n_ids == 0):
            # nothing to do.  (An EMPTY id list must not reach the library: its null data pointer would read as "no list = all texels" --
            # the case of a rank whose shard of a small texel list is empty, dist_util.shard_block_cyclic)
            return (out, st) if stats else out
        if ids is not None and n_ids >= 65536 and not getattr(self, "_tuned", False) and not torch.cuda.is_current_stream_capturing():
            # once per scene, before its first long launch: measure how full the scene's node steps run and pick the phase scheduler's weight
            # (texir_scene_tune: ~2 ms, blocking -- which is why it lives here and not inside the asynchronous texir_irt_generate)
            _lib.check(_lib.lib().texir_scene_tune(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, int(n_samples),
                                                   MODES[mode], _lib.stream_ptr()))
            self._tuned = int(n_samples) >= 256
        _lib.check(_lib.lib().texir_irt_generate(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, Nt,
                                                 int(n_samples), MODES[mode], _lib.ptr(out), _lib.ptr(st), _lib.stream_ptr()))
        return (out, st) if stats else out

    # -- irradiance split by source label (include/texir_hip.h texir_irt_split) ---------------------------
    def irt_split(self, pos, nrm, shift, n_samples, labels, n_classes, mode="uniform", texel_ids=None, unit=False, out=None, max_workspace_bytes=4 << 30):
        """per-class irradiance in one traced pass: labels [Ht,Wt] uint8 in the orientation of the scene's texture, n_classes in 1..8 -> out
        [n_classes, Nt, 3]; out[k] is bit for bit what irt_generate in its 64-texel form gives for the texture tex * [label == k] (unit=True: for the
        indicator texture of class k).  The id list is walked in slices that are multiples of 64 texels so that the partial-sum workspace stays
        under max_workspace_bytes; the cuts do not change a bit.  Only listed texels are written."""
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        K, N = int(n_classes), int(n_samples)
        if labels is not None:
            if not torch.is_tensor(labels):
                labels = torch.from_numpy(np.ascontiguousarray(labels))
            if labels.dtype != torch.uint8 or tuple(labels.shape) != tuple(self.tex_shape[:2]):
                raise ValueError("labels must be uint8 [%d,%d]" % tuple(self.tex_shape[:2]))
            labels = labels.to(device=self.device).contiguous()
        if out is None:
            out = torch.zeros((max(K, 0), Nt, 3), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (K, Nt, 3) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [%d,%d,3]" % (K, Nt))
        ids = None
        n = Nt
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n = ids.numel()
        if n == 0:
            return out
        L = _lib.lib()
        per_texel = int(L.texir_irt_split_workspace_bytes(1, N, K))       # (0 for arguments the library refuses: the call below then reports them)
        step = n
        if per_texel > 0 and per_texel * n > int(max_workspace_bytes):
            step = max(64, int(max_workspace_bytes) // per_texel // 64 * 64)
            if ids is None:
                ids = torch.arange(Nt, device=self.device, dtype=torch.int32)
        ws_bytes = max(per_texel * step, 16)
        ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8)
        for first in range(0, n, step):
            cnt = min(step, n - first)
            part = None if ids is None else ids[first:first + cnt]
            _lib.check(L.texir_irt_split(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(part), cnt, Nt, N, MODES[mode], _lib.ptr(labels),
                                         K, int(bool(unit)), _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
        return out

    # -- several radiance textures in one traced pass (include/texir_hip.h texir_irt_multi) ----------------
    def irt_multi(self, pos, nrm, shift, n_samples, textures, mode="uniform", texel_ids=None, out=None, max_workspace_bytes=4 << 30, interleaved=False):
        """the IrT estimator on K caller-owned textures in one traced pass: textures [K,Ht,Wt,3] float32 in the orientation (and of the size) of the
        scene's texture, K in 1..8 -> out [K, Nt, 3]; out[k] is bit for bit what irt_generate in its 64-texel form gives after set_texture(textures[k]).
        The scene's own texture is neither read nor changed.  interleaved=True: textures is [Ht,Wt,K,3], the form the kernel reads, and a contiguous
        float32 device tensor is used in place (a recorded graph replays with whatever it holds then); otherwise one permute().contiguous() makes that
        copy.  Any point list: texels or a view's pixels.  The id list is walked in slices that are multiples of 64 texels so that the partial-sum
        workspace stays under max_workspace_bytes; the cuts do not change a bit.  Only listed texels are written."""
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        N = int(n_samples)
        if not torch.is_tensor(textures):
            textures = torch.from_numpy(np.ascontiguousarray(textures, dtype=np.float32))
        Ht, Wt = (int(v) for v in self.tex_shape[:2])
        want = (Ht, Wt, -1, 3) if interleaved else (-1, Ht, Wt, 3)
        if textures.ndim != 4 or any(w >= 0 and int(s) != w for s, w in zip(textures.shape, want)):
            raise ValueError("textures must be %s, got %r" % ("[%d,%d,K,3] (interleaved)" % (Ht, Wt) if interleaved else "[K,%d,%d,3]" % (Ht, Wt), tuple(textures.shape)))
        K = int(textures.shape[2 if interleaved else 0])
        tex = textures.to(device=self.device, dtype=torch.float32)
        tex = tex.contiguous() if interleaved else tex.permute(1, 2, 0, 3).contiguous()
        if out is None:
            out = torch.zeros((K, Nt, 3), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (K, Nt, 3) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [%d,%d,3]" % (K, Nt))
        ids = None
        n = Nt
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n = ids.numel()
        if n == 0:
            return out
        L = _lib.lib()
        per_texel = int(L.texir_irt_multi_workspace_bytes(1, N, K))       # (0 for arguments the library refuses: the call below then reports them)
        step = n
        if per_texel > 0 and per_texel * n > int(max_workspace_bytes):
            step = max(64, int(max_workspace_bytes) // per_texel // 64 * 64)
            if ids is None:
                ids = torch.arange(Nt, device=self.device, dtype=torch.int32)
        ws_bytes = max(per_texel * step, 16)
        ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8)
        for first in range(0, n, step):
            cnt = min(step, n - first)
            part = None if ids is None else ids[first:first + cnt]
            _lib.check(L.texir_irt_multi(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(part), cnt, Nt, N, MODES[mode], _lib.ptr(tex) if K else None,
                                         K, _lib.ptr(out) if K else None, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
        return out

    # -- the shadow of inserted emitters' bodies on the captured light (include/texir_hip.h texir_irt_shadow) --
    def irt_shadow(self, pos, nrm, shift, n_samples, bodies, sets=None, mode="uniform", texel_ids=None, out=None, stats=False, max_workspace_bytes=4 << 30):
        """what the bodies of inserted emitters take from the captured irradiance: bodies [K,16] float32 records (irtlight.pack; a device tensor is used
        in place, so a recorded graph replays with whatever the records hold then), K <= 8; sets: M <= 8 lists of body indices (default: one set per
        body, [[0], [1], ...]), or a uint32-valued integer tensor of M bit masks, used in place when it is an int32 device tensor -> lost [M, Nt, 3]:
        lost[m] is the part of irt_generate's irradiance that arrived along rays a body of set m now intercepts (a union over the set, not a sum), so the
        relit irradiance is max(E - lost[m], 0) + the lights' own terms (irtlight.add(..., lost=)).  Any point list: texels or a view's pixels.  The id
        list is walked in slices that are multiples of 64 texels so that the partial-sum workspace stays under max_workspace_bytes; the cuts do not
        change a bit.  Only listed texels are written.  stats=True: also int64 [2] = (samples whose ray met a body: the rays traced, blocked ones)"""
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        N = int(n_samples)
        bodies = _dev_f32(bodies, self.device)
        if bodies.ndim != 2 or bodies.shape[1] != 16:
            raise ValueError("bodies must be [K,16], got %r" % (tuple(bodies.shape),))
        K = int(bodies.shape[0])
        if sets is None:
            sets = [[k] for k in range(K)]
        if torch.is_tensor(sets):
            masks = sets.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            bits = []
            for m, members in enumerate(sets):
                v = 0
                for k in members:
                    if not 0 <= int(k) < 32:
                        raise ValueError("set %d names body %r: indices are 0..31 (bits at or above K are ignored)" % (m, k))
                    v |= 1 << int(k)
                bits.append(v - (1 << 32) if v >= 1 << 31 else v)
            masks = torch.tensor(bits, dtype=torch.int32).reshape(-1).to(self.device)
        M = int(masks.numel())
        if out is None:
            out = torch.zeros((M, Nt, 3), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (M, Nt, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [%d,%d,3] on %s" % (M, Nt, self.device))
        st = torch.zeros(2, device=self.device, dtype=torch.int64) if stats else None
        ids = None
        n = Nt
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n = ids.numel()
        if n == 0:
            return (out, st) if stats else out
        L = _lib.lib()
        per_texel = int(L.texir_irt_shadow_workspace_bytes(1, N, M))      # (0 for arguments the library refuses: the call below then reports them)
        step = n
        if per_texel > 0 and per_texel * n > int(max_workspace_bytes):
            step = max(64, int(max_workspace_bytes) // per_texel // 64 * 64)
            if ids is None:
                ids = torch.arange(Nt, device=self.device, dtype=torch.int32)
        ws_bytes = max(per_texel * step, 16)
        ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8)
        for first in range(0, n, step):
            cnt = min(step, n - first)
            part = None if ids is None else ids[first:first + cnt]
            _lib.check(L.texir_irt_shadow(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(part), cnt, Nt, N, MODES[mode], _lib.ptr(bodies) if K else None,
                                          K, _lib.ptr(masks) if M else None, M, _lib.ptr(out) if M else None, _lib.ptr(st), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
        return (out, st) if stats else out

    # -- the shadow of inserted mesh objects on the captured light (include/texir_hip.h texir_irt_shadow_mesh) --
    @classmethod
    def occluder(cls, verts, tris, device=None):
        """a geometry-only handle for irt_shadow_mesh: verts [V,3], tris [T,3] in OBJECT space (dummy uvs, a 1 x 1 texture)"""
        tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        return cls(verts, tris, np.zeros((3 * tris.shape[0], 2), np.float32), np.zeros((1, 1, 3), np.float32), device=device)

    def bounds(self):
        """(lo [3], hi [3]) float32: the box of the vertices the triangles name (texir_scene_bounds)"""
        out = np.zeros(6, np.float32)
        _lib.check(_lib.lib().texir_scene_bounds(self.h, _lib.ptr(out)))
        return out[:3].copy(), out[3:].copy()

    def irt_shadow_mesh(self, pos, nrm, shift, n_samples, occluders, instances, poses, sets=None, mode="uniform", texel_ids=None, out=None, stats=False,
                        prefilter=True, max_workspace_bytes=4 << 30):
        """what inserted triangle-mesh objects take from the captured irradiance: occluders: Q <= 8 handles of Scene.occluder; instances: K <= 8 indices
        into them (instance j shows occluder instances[j]; an occluder may stand in the room twice); poses: [K,3,4] OBJECT-TO-WORLD on the host (numpy
        or a CPU tensor; inverted in float64 and rounded once, a singular pose is a ValueError), or a [K,12] WORLD-TO-OBJECT float32 DEVICE tensor, used in
        place (a recorded graph replays with whatever it holds then); sets: as irt_shadow's, over the instances (default: one set per instance) -> lost
        [M, Nt, 3]: lost[m] is the part of irt_generate's irradiance that arrived along rays an instance of set m now intercepts (a union, not a sum), so
        the irradiance with the objects in the room is max(E - lost[m], 0) (irtlight.add(..., lost=)).  Any point list: texels or a view's pixels.  The
        id list is walked in slices that are multiples of 64 texels so that the workspace stays under max_workspace_bytes; the cuts do not change a bit.
        Only listed texels are written.  prefilter=False: every lane queries every instance (the same bits, slower).  stats=True: also int64 [3] =
        (samples whose ray met some box: the scene rays traced, occluder queries, blocked samples)"""
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        N = int(n_samples)
        occluders, handles, Q, inst, w2o, K = mesh_instances(self.device, occluders, instances, poses)
        if sets is None:
            sets = [[k] for k in range(K)]
        if torch.is_tensor(sets):
            masks = sets.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            bits = []
            for m, members in enumerate(sets):
                v = 0
                for k in members:
                    if not 0 <= int(k) < 32:
                        raise ValueError("set %d names instance %r: indices are 0..31 (bits at or above K are ignored)" % (m, k))
                    v |= 1 << int(k)
                bits.append(v - (1 << 32) if v >= 1 << 31 else v)
            masks = torch.tensor(bits, dtype=torch.int32).reshape(-1).to(self.device)
        M = int(masks.numel())
        if out is None:
            out = torch.zeros((M, Nt, 3), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (M, Nt, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [%d,%d,3] on %s" % (M, Nt, self.device))
        st = torch.zeros(3, device=self.device, dtype=torch.int64) if stats else None
        ids = None
        n = Nt
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n = ids.numel()
        if n == 0:
            return (out, st) if stats else out
        L = _lib.lib()
        per_texel = int(L.texir_irt_shadow_mesh_workspace_bytes(1, N, M))      # (0 for arguments the library refuses: the call below then reports them)
        step = n
        if per_texel > 0 and per_texel * n > int(max_workspace_bytes):
            step = max(64, int(max_workspace_bytes) // per_texel // 64 * 64)
            if ids is None:
                ids = torch.arange(Nt, device=self.device, dtype=torch.int32)
        ws_bytes = max(per_texel * step, 16)
        ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8)
        for first in range(0, n, step):
            cnt = min(step, n - first)
            part = None if ids is None else ids[first:first + cnt]
            _lib.check(L.texir_irt_shadow_mesh(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(part), cnt, Nt, N, MODES[mode],
                                               C.cast(handles, C.c_void_p) if Q else None, Q, _lib.ptr(inst) if K else None, _lib.ptr(w2o) if K else None, K,
                                               _lib.ptr(masks) if M else None, M, _lib.ptr(out) if M else None, _lib.ptr(st), 0 if prefilter else 1, _lib.ptr(ws),
                                               ws_bytes, _lib.stream_ptr()))
        return (out, st) if stats else out

    # -- inserted emitters (include/texir_hip.h texir_irt_lights) ------------------------------------------
    def irt_lights(self, pos, nrm, shift, lights, n_samples, texel_ids=None, t_max=0.999, out=None, stats=False, query="closest", occluders=None, instances=None,
                   poses=None, prefilter=True):
        """direct irradiance factors of inserted area lights: lights [K,16] float32 records (irtlight.pack; a device tensor is used in place, so a
        recorded graph replays with whatever the records hold then), K <= 8 -> F [K, Nt]; the irradiance under emitted radiance c_k is c_k * F[k]
        (irtlight.add).  Any point list: texels or a view's pixels.  t_max: the ray is occluded iff its closest hit has t < t_max in units of the
        segment to the sample point (0.999: a light laid onto a surface is not shadowed by it).  Only listed texels are written.
        stats=True: also int64 [2] = (rays traced, visible ones).  query: 'closest' | 'any' (texir_irt_lights_any: visibility as an occlusion query, the
        same bits).  occluders, instances, poses, prefilter: inserted mesh objects that shadow the lights, with the meaning, host / device forms and
        float64 inversion of irt_shadow_mesh (texir_irt_lights_mesh: a segment is also blocked by an instance's triangles inside (0, t_max)).
        occluders=None calls the entry points above exactly as before; with occluders every question is an occlusion query, so `query` is accepted (and
        checked) but ignored -- the bits do not depend on it.  prefilter=False: every lane asks every instance (the same bits, slower)"""
        call = "texir_irt_lights_any" if check_query(query) else "texir_irt_lights"
        mesh = None if occluders is None else mesh_instances(self.device, occluders, instances, poses)
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        Nt = pos.shape[0]
        shift = _dev_f32(shift, self.device).reshape(Nt, 2)
        lights = _dev_f32(lights, self.device)
        if lights.ndim != 2 or lights.shape[1] != 16:
            raise ValueError("lights must be [K,16], got %r" % (tuple(lights.shape),))
        K = lights.shape[0]
        if out is None:
            out = torch.zeros((K, Nt), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (K, Nt) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [%d,%d] on %s" % (K, Nt, self.device))
        ids = None
        n_ids = 0
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n_ids = ids.numel()
        st = torch.zeros(2, device=self.device, dtype=torch.int64) if stats else None
        empty = Nt == 0 or (texel_ids is not None and n_ids == 0)          # (an EMPTY id list must not reach the library as "no list = all texels")
        if not empty and mesh is not None:
            _, handles, Q, inst, w2o, J = mesh
            _lib.check(_lib.lib().texir_irt_lights_mesh(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, Nt,
                                                        _lib.ptr(lights) if K else None, K, int(n_samples), float(t_max), C.cast(handles, C.c_void_p) if Q else None,
                                                        Q, _lib.ptr(inst) if J else None, _lib.ptr(w2o) if J else None, J, 0 if prefilter else 1,
                                                        _lib.ptr(out) if K else None, _lib.ptr(st), _lib.stream_ptr()))
        elif not empty:
            _lib.check(getattr(_lib.lib(), call)(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, Nt,
                                                 _lib.ptr(lights) if K else None, K, int(n_samples), float(t_max), _lib.ptr(out) if K else None, _lib.ptr(st),
                                                 _lib.stream_ptr()))
        return (out, st) if stats else out


    # -- the specular response to inserted emitters (include/texir_hip.h texir_spec_lights) -----------------
    def spec_lights(self, pos, nrm, rough, shift, cam, lights, n_samples, texel_ids=None, t_max=0.999, clamp_eps=1e-14, query="closest", out=None, stats=False,
                    occluders=None, instances=None, poses=None, prefilter=True):
        """specular (GGX) response factors of inserted area lights per pixel: pos, nrm [P,3] (pos already offset), rough [P], shift [P,2] (the pixels'
        specular shift), cam [3], lights [K,16] float32 records (irtlight.pack; a device tensor is used in place, as is a device cam, so a recorded graph
        replays with whatever they hold then), K <= 8 -> R [K, P]; the radiance a light of colour c_k adds to the view is c_k * R[k] beside its diffuse
        albedo / pi * c_k * F[k] (irtlight.add_view).  Balance-heuristic multiple importance sampling over the light's area and the GGX lobe, n_samples
        points each.  t_max, query, stats, out, texel_ids (here: pixel ids): as irt_lights.  clamp_eps: the material model's floor of denominators.
        occluders, instances, poses, prefilter: inserted mesh objects that shadow the lights, as irt_lights takes them (texir_spec_lights_mesh); with
        occluders `query` is accepted but ignored."""
        call = "texir_spec_lights_any" if check_query(query) else "texir_spec_lights"
        mesh = None if occluders is None else mesh_instances(self.device, occluders, instances, poses)
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        P = pos.shape[0]
        rough = _dev_f32(rough, self.device).reshape(P)
        shift = _dev_f32(shift, self.device).reshape(P, 2)
        cam = _dev_f32(cam, self.device).reshape(3)
        lights = _dev_f32(lights, self.device)
        if lights.ndim != 2 or lights.shape[1] != 16:
            raise ValueError("lights must be [K,16], got %r" % (tuple(lights.shape),))
        K = lights.shape[0]
        if out is None:
            out = torch.zeros((K, P), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (K, P) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [%d,%d] on %s" % (K, P, self.device))
        ids = None
        n_ids = 0
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n_ids = ids.numel()
        st = torch.zeros(2, device=self.device, dtype=torch.int64) if stats else None
        empty = P == 0 or (texel_ids is not None and n_ids == 0)           # (an EMPTY id list must not reach the library as "no list = all pixels")
        if not empty and mesh is not None:
            _, handles, Q, inst, w2o, J = mesh
            _lib.check(_lib.lib().texir_spec_lights_mesh(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(rough), _lib.ptr(shift), _lib.ptr(cam), _lib.ptr(ids), n_ids,
                                                         P, _lib.ptr(lights) if K else None, K, int(n_samples), float(t_max), float(clamp_eps),
                                                         C.cast(handles, C.c_void_p) if Q else None, Q, _lib.ptr(inst) if J else None,
                                                         _lib.ptr(w2o) if J else None, J, 0 if prefilter else 1, _lib.ptr(out) if K else None, _lib.ptr(st),
                                                         _lib.stream_ptr()))
        elif not empty:
            _lib.check(getattr(_lib.lib(), call)(self.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(rough), _lib.ptr(shift), _lib.ptr(cam), _lib.ptr(ids), n_ids, P,
                                                 _lib.ptr(lights) if K else None, K, int(n_samples), float(t_max), float(clamp_eps),
                                                 _lib.ptr(out) if K else None, _lib.ptr(st), _lib.stream_ptr()))
        return (out, st) if stats else out

    # -- the shadow of inserted bodies and mesh objects in the specular term of captured light (include/texir_hip.h texir_spec_shadow) --
    def spec_shadow(self, pos, nrm, rough, shift, cam, n_samples, bodies=None, occluders=None, instances=None, poses=None, sets=None, texel_ids=None,
                    clamp_eps=1e-14, prefilter=True, out=None, stats=False):
        """what inserted bodies and mesh objects take from the SPECULAR term of the captured light per pixel: pos, nrm [P,3] (pos already offset, nrm raw),
        rough [P], shift [P,2] (the pixels' specular shift), cam [3] and n_samples as spec_render takes them; bodies [Kb,16] float32 records (irtlight.pack,
        Kb <= 8; a device tensor is used in place); occluders, instances, poses as irt_shadow_mesh takes them (host object-to-world poses are inverted in
        float64, a singular one is a ValueError; a device [J,12] world-to-object tensor is used in place); sets: M <= 8 items, each an int mask (bit k = body
        k, bit 8 + j = instance j) or a pair (body indices, instance indices) -- spec_shadow_sets -- or an int32 device tensor of M masks, used in place;
        None: one set holding every body and every instance -> lost [M, P, 3]: lost[m] is the part of spec_render's specular term (irr = 0, albedo = 0) that
        arrived along rays a body or an instance of set m now intercepts, a union, not a sum; the relit pixel is max(rgb - lost[m], 0)
        (irtlight.add_view(lost_spec=)).  texel_ids: pixel ids, only listed pixels are written.  prefilter=False: every lane asks every instance (the same
        bits, slower).  stats=True: also int64 [3] = (samples whose ray met a body or a box: the scene rays traced, occluder queries, blocked samples)"""
        pos = _dev_f32(pos, self.device).reshape(-1, 3)
        nrm = _dev_f32(nrm, self.device).reshape(-1, 3)
        P = pos.shape[0]
        rough = _dev_f32(rough, self.device).reshape(P)
        shift = _dev_f32(shift, self.device).reshape(P, 2)
        cam = _dev_f32(cam, self.device).reshape(3)
        bodies = _dev_f32(np.zeros((0, 16), np.float32) if bodies is None else bodies, self.device)
        if bodies.ndim != 2 or bodies.shape[1] != 16:
            raise ValueError("bodies must be [Kb,16], got %r" % (tuple(bodies.shape),))
        Kb = int(bodies.shape[0])
        _, handles, Q, inst, w2o, J = mesh_instances(self.device, [] if occluders is None else occluders, instances, poses)
        if torch.is_tensor(sets):
            masks = sets.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            bits = spec_shadow_sets(sets, Kb, J)
            masks = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in bits], dtype=torch.int32).reshape(-1).to(self.device)
        M = int(masks.numel())
        if out is None:
            out = torch.zeros((M, P, 3), device=self.device, dtype=torch.float32)
        elif tuple(out.shape) != (M, P, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [%d,%d,3] on %s" % (M, P, self.device))
        ids = None
        n_ids = 0
        if texel_ids is not None:
            ids = texel_ids.to(device=self.device, dtype=torch.int32).contiguous()
            n_ids = ids.numel()
        st = torch.zeros(3, device=self.device, dtype=torch.int64) if stats else None
        empty = P == 0 or (texel_ids is not None and n_ids == 0)           # (an EMPTY id list must not reach the library as "no list = all pixels")
        if not empty:
            _lib.check(_lib.lib().texir_spec_shadow(self.h, _lib.ptr(nrm), _lib.ptr(rough), _lib.ptr(pos), _lib.ptr(cam), _lib.ptr(shift), _lib.ptr(ids), n_ids, P,
                                                    int(n_samples), float(clamp_eps), _lib.ptr(bodies) if Kb else None, Kb,
                                                    C.cast(handles, C.c_void_p) if Q else None, Q, _lib.ptr(inst) if J else None, _lib.ptr(w2o) if J else None, J,
                                                    _lib.ptr(masks) if M else None, M, 0 if prefilter else 1, _lib.ptr(out) if M else None, _lib.ptr(st),
                                                    _lib.stream_ptr()))
        return (out, st) if stats else out


def generate_dir(normals, num_sample_dir, shift, mode="uniform", roughness=None):
    """utils/sample_util.py:63-146 on the GPU; `shift` [b,2] is the torch.rand(b,1,2) of :102 made explicit."""
    dev = normals.device
    normals = normals.to(torch.float32).contiguous().reshape(-1, 3)
    b = normals.shape[0]
    shift = _dev_f32(shift, dev).reshape(b, 2)
    r = None if roughness is None else roughness.to(torch.float32).contiguous().reshape(b)
    L = torch.empty((b, num_sample_dir, 3), device=dev, dtype=torch.float32)
    if b == 0:
        return L
    _lib.check(_lib.lib().texir_generate_dir(_lib.ptr(normals), _lib.ptr(r), _lib.ptr(shift), b, int(num_sample_dir), MODES[mode],
                                             _lib.ptr(L), _lib.stream_ptr()))
    return L


def spec_forward_raw(scene, normal, albedo, rough, points, irr, cam, shift, S, clamp_eps=1e-14, lighting=None, want_dw=False):
    """texir_spec_forward on contiguous float32 tensors (no autograd): -> (rgb [P,3], Ls [P,S,3] = the traced -- or given -- lighting the backward needs,
    dw [P,S] | None = the sample weights' derivatives wrt roughness when want_dw: the training form, texir_spec_forward_train)"""
    P = normal.shape[0]
    rgb = torch.empty((P, 3), device=normal.device, dtype=torch.float32)
    # lighting given: specular_reflectance on the caller's radiance (no tracing); else traced and kept for the backward
    Ls = torch.empty((P, S, 3), device=normal.device, dtype=torch.float32) if lighting is None else lighting
    dw = torch.empty((P, S), device=normal.device, dtype=torch.float32) if want_dw else None
    if P > 0:
        L = _lib.lib()
        head = (None if scene is None else scene.h, _lib.ptr(normal), _lib.ptr(albedo), _lib.ptr(rough), _lib.ptr(points), _lib.ptr(irr), _lib.ptr(cam), _lib.ptr(shift),
                P, S, float(clamp_eps), 0 if lighting is None else 1, _lib.ptr(rgb), _lib.ptr(Ls))
        if want_dw:
            _lib.check(L.texir_spec_forward_train(*head, _lib.ptr(dw), _lib.stream_ptr()))
        else:
            _lib.check(L.texir_spec_forward(*head, _lib.stream_ptr()))
    return rgb, Ls, dw


def spec_backward_raw(normal, rough, points, irr, cam, shift, Ls, d_rgb, S, clamp_eps=1e-14, need_albedo=True, need_rough=True, dw=None):
    """d rgb -> (d albedo [P,3] | None, d roughness [P] | None), no autograd.  dw (from spec_forward_raw(want_dw=True)): texir_spec_backward_ws, a stream over
    what the forward kept; else texir_spec_backward, which recomputes the sample chain"""
    P = normal.shape[0]
    d_rgb = d_rgb.contiguous()
    d_a = torch.empty((P, 3), device=normal.device, dtype=torch.float32) if need_albedo else None
    d_r = torch.empty((P,), device=normal.device, dtype=torch.float32) if need_rough else None
    if P > 0 and (need_albedo or need_rough):
        if dw is not None:
            _lib.check(_lib.lib().texir_spec_backward_ws(_lib.ptr(irr), _lib.ptr(Ls), _lib.ptr(dw), _lib.ptr(d_rgb), P, S, _lib.ptr(d_a), _lib.ptr(d_r), _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib().texir_spec_backward(_lib.ptr(normal), _lib.ptr(rough), _lib.ptr(points), _lib.ptr(irr), _lib.ptr(cam),
                                                      _lib.ptr(shift), _lib.ptr(Ls), _lib.ptr(d_rgb), P, S, float(clamp_eps), _lib.ptr(d_a), _lib.ptr(d_r),
                                                      _lib.stream_ptr()))
    return d_a, d_r


class _SpecRender(torch.autograd.Function):
    """render + specular_reflectance (mat_nvdiffrast.py:201-249,260-279) with its analytic backward."""

    @staticmethod
    def forward(ctx, scene, normal, albedo, rough, points, irr, cam, shift, S, clamp_eps=1e-14, lighting=None):
        # roughness is being optimised: keep the weights' derivatives the forward computes anyway, and the backward needs no second pass over the sample chain
        want_dw = bool(ctx.needs_input_grad[3]) and _TRAIN_FORM[0]
        rgb, Ls, dw = spec_forward_raw(scene, normal, albedo, rough, points, irr, cam, shift, S, clamp_eps, lighting, want_dw)
        ctx.save_for_backward(normal, rough, points, irr, cam, shift, Ls, dw)
        ctx.S, ctx.clamp_eps = S, float(clamp_eps)
        return rgb

    @staticmethod
    def backward(ctx, d_rgb):
        normal, rough, points, irr, cam, shift, Ls, dw = ctx.saved_tensors
        d_a, d_r = spec_backward_raw(normal, rough, points, irr, cam, shift, Ls, d_rgb, ctx.S, ctx.clamp_eps, ctx.needs_input_grad[2], ctx.needs_input_grad[3], dw)
        return None, None, d_a, d_r, None, None, None, None, None, None, None


# A/B switch (TEXIR_SPEC_TRAIN_FORM=0: the backward recomputes the sample chain, texir_spec_backward -- the round-3 form)
_TRAIN_FORM = [__import__("os").environ.get("TEXIR_SPEC_TRAIN_FORM", "1") != "0"]


def spec_shift_arg(shift, P, dev):
    """the `shift` argument of the specular kernels: a PINNED host tensor is handed over as it is (pinned allocations are mapped into the device's address
    space: a recorded hipGraph reads each step's freshly drawn shifts without a staging copy); anything else becomes a float32 device tensor"""
    if torch.is_tensor(shift) and shift.device.type == "cpu" and shift.is_pinned() and shift.dtype == torch.float32 and shift.is_contiguous() and shift.numel() == 2 * P:
        return shift.reshape(P, 2)
    return shift.to(device=dev, dtype=torch.float32).reshape(P, 2).contiguous()


def spec_render(scene, normal, albedo, roughness, points, irr, cam_position, shift, num_samples, clamp_eps=1e-14, lighting=None):
    """rgb [P,3] = irr*albedo/pi + GGX specular; differentiable wrt albedo [P,3] and roughness [P] / [P,1].
    clamp_eps: floor of the BRDF denominators (1e-14 in mat_nvdiffrast.py, 1e-6 in the evaluation model test_nvdiffrast.py).
    lighting [P,S,3]: use the caller's radiance instead of tracing (the specular_reflectance function seam; scene may be None)."""
    dev = scene.device if scene is not None else normal.device
    P = normal.reshape(-1, 3).shape[0]
    f = lambda t, s: t.to(device=dev, dtype=torch.float32).reshape(*s).contiguous()
    S = int(num_samples)
    sh = spec_shift_arg(shift, P, dev)
    return _SpecRender.apply(scene, f(normal, (P, 3)), f(albedo, (P, 3)), f(roughness, (P,)), f(points, (P, 3)), f(irr, (P, 3)),
                             f(cam_position, (3,)), sh, S, float(clamp_eps), None if lighting is None else f(lighting, (P, S, 3)))


def diffuse_irradiance(scene, points, normals, shift, num_samples, sample_type="uniform"):
    """the lighting integral of diffuse_reflectance (mat_nvdiffrast.py:252-258): diffuse_reflectance(query_irf(...), l, n, albedo, type)/N
    == diffuse_irradiance(...) * albedo / pi.  points (already offset) / normals [P,3], shift [P,2] -> [P,3]"""
    dev = scene.device
    P = points.reshape(-1, 3).shape[0]
    f = lambda t, s: t.to(device=dev, dtype=torch.float32).reshape(*s).contiguous()
    out = torch.empty((P, 3), device=dev, dtype=torch.float32)
    if P == 0:
        return out
    _lib.check(_lib.lib().texir_diffuse_irradiance(scene.h, _lib.ptr(f(points, (P, 3))), _lib.ptr(f(normals, (P, 3))), _lib.ptr(f(shift, (P, 2))), P,
                                                   int(num_samples), MODES[sample_type], _lib.ptr(out), _lib.stream_ptr()))
    return out
