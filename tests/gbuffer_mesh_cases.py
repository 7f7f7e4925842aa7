"""Cases of the instanced cube G-buffer (include/texir_hip.h texir_gbuffer_cast_mesh, csrc/gbuffermesh.hip; gbuffer.cast_gbuffer(occluders=...)): the float64
reference of a pixel, the checker, a float32 restatement of the rule with the mutants the checker must reject, and the seeded cases.  Shared by
test_gbuffer_mesh_ref_cpu.py (no GPU) and test_gpu_gbuffer_mesh.py; no tests here.  K = 4, U = 2^-24 and TINY are texture_cases'; the room's rays, candidates
and output bounds are gbuffer_cases.GRef's, unchanged; the object-space ray is built as irt_shadow_mesh_cases builds it; the occluders and poses are
irt_shadow_mesh_cases'.  Every bound was derived from the reference alone and written here before any GPU run; nothing is taken from a kernel's output.

THE REFERENCE OF A PIXEL.  The room's candidates: GRef.rays (trace_cases.RayRef over the room along the exact ray, its dir_bound = K (bound_arith(d) + the
fold of the eye's rounding)).  Per instance j a RayRef over the OCCLUDER's triangles along the object-space ray
    o' = the header's float32 sequence in numpy on the float32 eye of gbuffer_cases.basis_model (a fixed value on any IEEE machine)
    d' = W d in float64, with the bound |W| e_w + K 3 u |W| |d| of texir_irt_shadow_mesh, where e_w is the pixel's own dir_bound: K (bound_arith(d) +
         e(eye) |d| / (D_j - |e(eye)|)), D_j the float64 distance from the exact eye to the posed instance (the fold of gbuffer_cases with the instance in the
         place of the room: the library's float32 eye may differ from basis_model's by e(eye) and no more).
A SURFACE is the room (-1) or an instance (0 .. J - 1).  An OUTCOME (surface, triangle) is ADMISSIBLE iff the triangle is in the surface's candidate list
(check_hits' rule within the surface: a candidate that no robustly hit triangle of the same list shadows) and no OTHER surface has a robust hit that is
certainly nearer: t' + bound_t' < t - bound_t.  Background is admissible only where no surface has a robust hit (never inside a closed room: check_gbuffer's rule).  Exact ties (the scene wins, the lower
index wins) are beyond a float64 reference: both sides are admissible here, and the GPU module holds the tie rules bit for bit on constructed ties.

BOUNDS OF AN INSTANCE PIXEL, for the triangle (A, B, C) of occluder geometry the kernel chose, its reference t, bound_t (K included):
  position   reference eye32 + t d (the header's pos = eye + t d with the float32 eye, the exact direction).  The kernel's d is off by bound_arith(d), its t by
             bound_t, its eye by e(eye) at most; one product and one sum:
                 K (e(eye) + |t| bound_arith(d) + u |t d| + u |pos|) + |d| bound_t                         per axis
  normal     n_o, e(n_o) = gbuffer_cases.geometric_normal64 of (A, B, C) (the largest over the three stored rotations, without K).  With W the float32 matrix:
                 m_c = sum_r W[r][c] n_o,r     e(m_c) = sum_r |W[r][c]| e(n_o,r) + 3 u sum_r |W[r][c] n_o,r|   (three products, two sums)
                 q = m . m                     e(q) = 2 sum_c |m_c| e(m_c) + 3 u q                           (every term positive)
                 nrm_c = m_c rsq(q)            e = e(m_c) / |m| + |m_c| / |m| (e(q) / (2 q) + 5 u)             (rsq within 2 ulp = 4 u; the product)
             times K: the form of the geometric normal's own bound, one stage further.
  uv = (0, 0), uv_da = 0, mask = 1, tri_id = the occluder's own triangle + 1, inst_id = j: exact.
A pixel whose surface is the room (inst_id = -1) goes through gbuffer_cases.check_gbuffer with its own bounds; for that call the instance pixels are
filled with gbuffer_f32's room values, which test_gbuffer_ref_cpu.py proves pass.

CAPS (from the reference alone, asserted in test_gbuffer_mesh_ref_cpu.py): no candidate list overflows; at most CAP_MULTI = 2 % of a case's pixels have
admissible outcomes on more than one surface; every case not marked degenerate shows an instance alone on at least CAP_SHARE = 5 % of its pixels and the room
alone on at least 5 %; D_j >= 0.01.  The shares are printed.
"""
import numpy as np

import gbuffer_cases as GC
import irt_shadow_mesh_cases as MC
import trace_cases as TC
from texture_cases import K, TINY, U

F32, F64 = np.float32, np.float64
CAP_MULTI = TC.CAP_MULTI
CAP_SHARE = 0.05
D_INST_MIN = 0.01
KEYS = ("position", "normal", "mask", "uv", "uv_da", "tri_id", "inst_id")


# ---- a case ---------------------------------------------------------------------------------------------------------------------------------------------------

class Case:
    """base: a gbuffer_cases.Case (room, mvp, c, pix); occ: names of the Q occluders (irt_shadow_mesh_cases.occluder); inst: occluder index per instance;
    poses [J,3,4] object-to-world float64; degenerate: the share caps do not apply (the eye inside an instance)"""

    def __init__(self, name, base, occ, inst, poses, degenerate=False):
        self.name, self.base, self.occ, self.inst = name, base, list(occ), [int(i) for i in inst]
        self.poses = np.asarray(poses, F64).reshape(-1, 3, 4)
        self.J = len(self.inst)
        assert self.poses.shape[0] == self.J
        self.w2o = MC.to_world_to_object(self.poses) if self.J else np.zeros((0, 12), F32)
        self.degenerate = degenerate
        self.geo, self.c, self.mvp = base.geo, base.c, base.mvp
        self._ref = None

    def geos(self):
        return [MC.occluder(n) for n in self.occ]

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref


def eye32_of(base):
    """the float32 eye of every reference pixel [R,3]: gbuffer_cases.basis_model's value"""
    ref = base.ref()
    return np.stack([b.eye for b in ref.model]).astype(F32)[ref.face]


class Ref:
    def __init__(self, case):
        self.case = c = case
        self.g = g = c.base.ref()
        R = g.rays.R
        self.eye32 = eye32_of(c.base)
        e_eye = np.stack([b.e_eye for b in g.model])[g.face]
        self.e_eye = e_eye
        nd = np.linalg.norm(g.d, axis=1)
        self.rays, self.d_inst = [], []
        geos = c.geos()
        for j in range(c.J):
            og = geos[c.inst[j]]
            W = c.w2o[j].astype(F64).reshape(3, 4)
            A, t = c.poses[j][:, :3], c.poses[j][:, 3]
            Vw = og.verts.astype(F64)[og.tris] @ A.T + t
            dj = np.array([GC.point_mesh_distance(b.eye, Vw) for b in g.exact])
            self.d_inst.append(float(dj.min()))
            room = dj[g.face] - np.linalg.norm(e_eye, axis=1)
            assert (room > 0).all(), "the eye's own rounding reaches instance %d: move it" % j
            e_w = K * (g.bd + e_eye * (nd / room)[:, None])
            o32 = MC.point_f32(c.w2o[j], self.eye32).astype(F64)
            d_o = g.d @ W[:, :3].T
            bd_o = e_w @ np.abs(W[:, :3]).T + K * (3 * U * (np.abs(g.d) @ np.abs(W[:, :3]).T) + 3 * TINY)
            self.rays.append(TC.RayRef(og, o32, d_o, bd_o))
        # per surface (row 0: the room, row 1 + j: instance j): the upper end of its nearest robust hit, +inf without one
        surf = [g.rays] + self.rays
        lim = np.full((len(surf), R), np.inf)
        for s, ry in enumerate(surf):
            with np.errstate(invalid="ignore"):
                rob = ry.has & (ry.c["robust"] > 0)
                lim[s] = np.where(rob, ry.t + ry.bt, np.inf).min(1)
        self.lim = lim
        self.any_robust = np.isfinite(lim).any(0)
        # admissible outcomes per surface [S][R,C]: in the list, and no OTHER surface certainly nearer
        self.adm = []
        for s, ry in enumerate(surf):
            others = np.delete(lim, s, axis=0).min(0) if len(surf) > 1 else np.full(R, np.inf)
            with np.errstate(invalid="ignore"):
                self.adm.append(ry.has & (ry.t - ry.bt <= others[:, None]))
        self.surf_ok = np.stack([a.any(1) for a in self.adm])                       # [S,R]
        self.bg_ok = ~self.any_robust & (not c.base.closed)                          # (a closed room with the eye inside has no background: check_gbuffer's rule)
        self.single = (self.surf_ok.sum(0) + self.bg_ok) == 1                        # one admissible surface (background counts as one)

    def caps(self):
        """(lists that overflow, share of pixels with outcomes on more than one surface, share showing an instance alone, the room alone, smallest D_j)"""
        over = int(self.g.rays.overflow.sum()) + sum(int(r.overflow.sum()) for r in self.rays)
        n_s = self.surf_ok.sum(0) + self.bg_ok
        inst_only = self.surf_ok[1:].any(0) & ~self.surf_ok[0] & ~self.bg_ok if self.case.J else np.zeros(self.g.rays.R, bool)
        room_only = self.surf_ok[0] & ~self.surf_ok[1:].any(0) & ~self.bg_ok
        return over, float((n_s > 1).mean()), float(inst_only.mean()), float(room_only.mean()), min(self.d_inst) if self.d_inst else np.inf

    def instance_outputs(self, j, rows, k):
        """the reference of instance pixels: rays `rows`, candidate slots `k` of instance j -> {position, normal: (value [n,3], bound [n,3] with K)}"""
        c, g, ry = self.case, self.g, self.rays[j]
        og = c.geos()[c.inst[j]]
        t, bt = ry.t[rows, k], ry.bt[rows, k]
        d, bd = g.d[rows], g.bd[rows]
        pos = self.eye32[rows].astype(F64) + t[:, None] * d
        e_pos = K * (self.e_eye[rows] + np.abs(t)[:, None] * bd + U * np.abs(t[:, None] * d) + U * np.abs(pos) + 2 * TINY) + np.abs(d) * bt[:, None]
        P = og.verts.astype(F64)[og.tris[ry.id[rows, k].astype(np.int64)]]
        n_o, e_no = GC.geometric_normal64(P)
        W3 = c.w2o[j].astype(F64).reshape(3, 4)[:, :3]
        m = n_o @ W3
        e_m = e_no @ np.abs(W3) + 3 * U * (np.abs(n_o) @ np.abs(W3)) + 3 * TINY
        q = (m * m).sum(1)
        e_q = 2 * (np.abs(m) * e_m).sum(1) + 3 * U * q + 3 * TINY
        with np.errstate(divide="ignore", invalid="ignore"):
            ln = np.sqrt(q)
            unit = m / ln[:, None]
            e_n = e_m / ln[:, None] + np.abs(unit) * (e_q / (2 * q) + 5 * U)[:, None] + TINY
        return {"position": (pos, e_pos), "normal": (unit, K * e_n)}


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------------------------------

_FILL = {}


def _room_fill(base, cn, flip_v):
    """gbuffer_f32's room values of the base case (what stands in for the instance pixels when the room's pixels go through check_gbuffer)"""
    key = (base.name, None if cn is None else np.asarray(cn).tobytes(), int(flip_v))
    if key not in _FILL:
        _FILL[key] = GC.gbuffer_f32(base, cn, flip_v)
    return _FILL[key]


def check(case, out, cn, flip_v, family="gbm", what=""):
    """out: dict of numpy arrays over ALL 6 c c pixels (KEYS); cn: the corner normals the room holds (None: never set) -> dict output -> worst error / bound;
    raises AssertionError naming the pixels that fail and why"""
    ref = case.ref()
    g, P, J = ref.g, 6 * case.c * case.c, case.J
    what = "%s flip_v=%d %s" % (case.name, flip_v, what)
    inst_all = np.asarray(out["inst_id"]).reshape(-1).astype(np.int64)
    tri_all = np.asarray(out["tri_id"]).reshape(-1).astype(np.int64)
    mask_all = np.asarray(out["mask"], F64).reshape(-1)
    assert inst_all.shape == (P,) and tri_all.shape == (P,) and mask_all.shape == (P,)
    assert ((inst_all >= -1) & (inst_all < J)).all(), "%s: inst_id outside [-1, J)" % what
    assert (mask_all == (tri_all > 0)).all(), "%s: mask is not (tri_id > 0)" % what
    pix = g.pix
    inst, tri = inst_all[pix], tri_all[pix]
    rr = np.arange(len(pix))
    # the room's pixels: admissible across the surfaces, then gbuffer_cases' own check
    room = inst < 0
    ry = g.rays
    pid = tri - 1
    match = ry.has & (ry.id == pid[:, None]) & (pid >= 0)[:, None]
    found, k = match.any(1), match.argmax(1)
    hidden = room & found & ~ref.adm[0][rr, k]
    assert not hidden.any(), "%s: %d pixels show the room where an instance is certainly nearer, first pixel %d" % (what, int(hidden.sum()), pix[hidden][0])
    bg_bad = room & (tri == 0) & ~ref.bg_ok
    assert not bg_bad.any(), "%s: %d background pixels where a surface is robustly hit, first pixel %d" % (what, int(bg_bad.sum()), pix[bg_bad][0])
    fill = _room_fill(case.base, cn, flip_v)
    merged = {}
    on_inst = inst_all >= 0
    for name in GC.OUTPUTS + ("mask", "tri_id"):
        a = np.asarray(out[name]).reshape(P, -1).copy()
        a[on_inst] = np.asarray(fill[name]).reshape(P, -1)[on_inst]
        merged[name] = a.reshape(P) if name in ("mask", "tri_id") else a
    worst = GC.check_gbuffer(case.base, merged, cn, flip_v, family, what)
    # the instances' pixels
    got = {name: np.asarray(out[name], F64).reshape(P, -1)[pix] for name in GC.OUTPUTS}
    for j in range(J):
        rows = np.nonzero(inst == j)[0]
        if not rows.size:
            continue
        ryj, og = ref.rays[j], case.geos()[case.inst[j]]
        pj = tri[rows] - 1
        assert ((pj >= 0) & (pj < og.T)).all(), "%s: tri_id of an instance %d pixel outside [1, T]" % (what, j)
        mt = ryj.has[rows] & (ryj.id[rows] == pj[:, None])
        fj, kj = mt.any(1), mt.argmax(1)
        assert fj.all(), "%s: %d pixels of instance %d name a triangle that is no candidate of the ray, first pixel %d triangle %d" % (
            what, int((~fj).sum()), j, pix[rows[~fj][0]], pj[~fj][0])
        ok = ref.adm[1 + j][rows, kj]
        assert ok.all(), "%s: %d pixels show instance %d where another surface is certainly nearer, first pixel %d" % (what, int((~ok).sum()), j, pix[rows[~ok][0]])
        exact = (got["uv"][rows] == 0).all(1) & (got["uv_da"][rows] == 0).all(1)
        assert exact.all(), "%s: uv / uv_da of %d instance %d pixels are not exactly zero, first pixel %d" % (what, int((~exact).sum()), j, pix[rows[~exact][0]])
        want = ref.instance_outputs(j, rows, kj)
        for name in ("position", "normal"):
            val, bnd = want[name]
            assert np.isfinite(got[name][rows]).all(), "%s: non-finite %s on instance %d" % (what, name, j)
            err = np.abs(got[name][rows] - val)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / bnd)
            bad = ~(ratio <= 1)
            w = float(ratio.max()) if not bad.any() else np.inf
            fam = family + "_inst_" + ("pos" if name == "position" else "nrm")
            TC._note(fam, what + " instance %d" % j, w)
            worst[fam] = max(worst.get(fam, 0.0), w)
            if bad.any():
                n, col = np.argwhere(bad)[0]
                raise AssertionError("%s: %s of instance %d outside its bound at %d of %d values; pixel %d triangle %d entry %d: got %r, reference %r, bound %.3e"
                                     % (what, name, j, int(bad.sum()), bad.size, pix[rows[n]], pj[n], col, float(got[name][rows[n], col]), float(val[n, col]),
                                        float(bnd[n, col])))
    return worst


# ---- the float32 restatement of the header's rule (CPU) ---------------------------------------------------------------------------------------------------------------

MUTANTS = ("w_not_transposed", "not_normalised", "mirror_flipped", "object_space_pos", "unbounded", "last_wins", "inst_off_by_one", "tri_no_plus_1", "uv_not_zero",
           "uv_da_kept")


def rays_f32(base):
    """eye, d [R,3] float32 of the reference pixels as gbuffer_f32 forms them"""
    ref = base.ref()
    face, i, j = GC.pixel_grid(base.c, ref.pix)
    g = lambda name: np.stack([getattr(b, name) for b in ref.model]).astype(F32)[face]
    eye, d0, bx, by = g("eye"), g("d0"), g("dx"), g("dy")
    cf = F32(base.c)
    x = (j.astype(F32) + F32(0.5)) / cf * F32(2) - F32(1)
    y = (i.astype(F32) + F32(0.5)) / cf * F32(2) - F32(1)
    return eye, (d0 + x[:, None] * bx + y[:, None] * by).astype(F32)


def _normalise32(n):
    il = (F32(1) / np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F64))).astype(F32)
    return (n * il[:, None]).astype(F32)


def gbuffer_mesh_f32(case, cn, flip_v, mut=None):
    """texir_gbuffer_cast_mesh in numpy float32 over the reference pixels: the room by gbuffer_f32, its t by _isect_f32 on the triangle it chose; per instance
    in index order the first-ranked candidate of its RayRef, its t by _isect_f32 along the float32 object-space ray, accepted iff 0 < t < t_best.  mut: MUTANTS"""
    base, ref = case.base, case.ref()
    g = ref.g
    P = 6 * case.c * case.c
    out = {k: np.array(v, copy=True) for k, v in GC.gbuffer_f32(base, cn, flip_v).items()}
    out["inst_id"] = np.full(P, -1, np.int32)
    eye, d = rays_f32(base)
    pid = g.rays.id[:, 0].astype(np.int64)
    hit = pid >= 0
    V = base.geo.verts[base.geo.tris[np.where(hit, pid, 0)]]
    with np.errstate(all="ignore"):
        ts, _, _ = GC._isect_f32(eye, d, V)
    t_scene = np.where(hit, ts, np.inf).astype(F32)
    t_best = t_scene.copy()
    R = len(pid)
    surf = np.full(R, -1, np.int64)
    pos, nrm, tri = np.zeros((R, 3), F32), np.zeros((R, 3), F32), np.zeros(R, np.int64)
    geos = case.geos()
    for j in range(case.J):
        og, ry = geos[case.inst[j]], ref.rays[j]
        W = case.w2o[j].reshape(3, 4)
        o_o, d_o = MC.point_f32(case.w2o[j], eye), MC.dir_f32(case.w2o[j], d)
        pj = ry.id[:, 0].astype(np.int64)
        has = pj >= 0
        Vo = og.verts[og.tris[np.where(has, pj, 0)]]
        with np.errstate(all="ignore"):
            t, _, _ = GC._isect_f32(o_o, d_o, Vo)
            far = {"unbounded": np.full(R, np.inf, F32), "last_wins": t_scene}.get(mut, t_best)
            acc = has & (t > 0) & (t < far)
            e1, e2 = Vo[:, 1] - Vo[:, 0], Vo[:, 2] - Vo[:, 0]
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            n_o = _normalise32(n)
            W3 = W[:, :3] if mut == "w_not_transposed" else W[:, :3].T                  # m_c = sum_r W[r][c] n_o,r
            m = np.stack([(W3[c, 0] * n_o[:, 0] + W3[c, 1] * n_o[:, 1]) + W3[c, 2] * n_o[:, 2] for c in range(3)], 1).astype(F32)
            nj = m if mut == "not_normalised" else _normalise32(m)
            if mut == "mirror_flipped" and np.linalg.det(W[:, :3].astype(F64)) < 0:
                nj = -nj
            pj_w = (o_o + t[:, None] * d_o) if mut == "object_space_pos" else (eye + t[:, None] * d)
        surf[acc], tri[acc] = j, pj[acc] + (0 if mut == "tri_no_plus_1" else 1)
        pos[acc], nrm[acc] = pj_w[acc].astype(F32), nj[acc]
        if mut not in ("unbounded", "last_wins"):
            t_best = np.where(acc, t, t_best).astype(F32)
    on = np.nonzero(surf >= 0)[0]
    px = g.pix[on]
    out["position"][px], out["normal"][px] = pos[on], nrm[on]
    out["mask"][px], out["tri_id"][px] = 1, tri[on]
    out["inst_id"][px] = surf[on] + (1 if mut == "inst_off_by_one" else 0)
    if mut != "uv_not_zero":
        out["uv"][px] = 0
    if mut != "uv_da_kept":
        out["uv_da"][px] = 0
    return out


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------------------------------------------

EYES = {"centre": (0.0, 0.0, 0.0), "graze": GC.GRAZE}
AXIS = (1.0, 2.0, 0.5)
OFF = np.array([-0.5, -0.2, 0.3])                # from the eye to the middle of an arrangement: inside the cube [-1, 1]^3 from both eyes


def arrangement(kind, eye):
    """(occluder names, instance -> occluder, poses [J,3,4], degenerate) of one arrangement as seen from `eye`"""
    e = np.asarray(eye, F64)
    at = e + OFF
    if kind == "box":                                                               # a 12-triangle box under rotation and non-uniform scale
        return ["cube"], [0], [MC.pose(at, AXIS, 35.0, (0.7, 0.4, 0.5))], False
    if kind == "ico":                                                               # a level-1 icosphere of 80 triangles
        return ["ico"], [0], [MC.pose(at, (1, 2, 3), 35.0, 0.7)], False
    if kind == "twice":                                                             # one occluder shown twice under two poses
        return ["ico"], [0, 0], [MC.pose(at, (1, 2, 3), 35.0, 0.6), MC.pose(e + (-0.3, 0.3, -0.4), (3, 1, 2), 70.0, (0.5, 0.3, 0.4))], False
    if kind == "mirror":                                                            # a mirrored pose: negative determinant
        return ["cube"], [0], [MC.pose(at, AXIS, 35.0, (-0.7, 0.4, 0.5))], False
    if kind == "inter":                                                             # two interpenetrating instances
        # (the sphere, nearer the eye over most of the overlap, has the LOWER index: the last accepting instance is not the nearest)
        return ["ico", "cube"], [0, 1], [MC.pose(at + (0.12, 0.1, -0.05), (1, 2, 3), 35.0, 0.62), MC.pose(at, AXIS, 20.0, 0.5)], False
    if kind == "cut":                                                               # cut by the wall x = 1, and a second one wholly behind it
        return ["cube"], [0, 0], [MC.pose((0.85, -0.3, 0.3), (0, 1, 0), 0.0, 0.7), MC.pose((1.5, 0.2, -0.3), AXIS, 25.0, 0.5)], False
    if kind == "inside":                                                            # the eye inside the instance
        return ["ico"], [0], [MC.pose(e + (0.1, 0.0, 0.05), (1, 2, 3), 35.0, 1.0)], True
    if kind == "eight":                                                             # J = 8
        poses = [MC.pose(e + (-0.5, 0.25 * (k % 4) - 0.45, 0.3 * (k // 4) - 0.05), AXIS, 15.0 * k, 0.24) for k in range(8)]
        return ["cube", "ico"], [k % 2 for k in range(8)], poses, False
    raise KeyError(kind)


KINDS = ("box", "ico", "twice", "mirror", "inter", "cut", "inside", "eight")
BOX_NAMES = ["%s_%s_c%d" % (kind, eye, c) for kind in KINDS for eye in ("centre", "graze") for c in (8, 17)]
NAMES = BOX_NAMES + ["room_table_c16", "stride_c296"]
_CASES = {}


def _stride_instance(base):
    """an icosphere in view of the grid-stride loop's second trip: half way to the wall along the mean direction of those pixels, wide enough for a fifth of them"""
    ref = base.ref()
    rows = np.nonzero(ref.pix >= GC.STRIDE_START)[0]
    d = ref.d[rows] / np.linalg.norm(ref.d[rows], axis=1, keepdims=True)
    dm = d.mean(0) / np.linalg.norm(d.mean(0))
    t_wall = float(np.nanmin(ref.rays.t[rows, 0] * np.linalg.norm(ref.d[rows], axis=1)))
    s = 0.5 * t_wall
    return MC.pose(ref.eye[rows[0]] + s * dm, (1, 2, 3), 35.0, 0.5 * s)               # radius s / 4: about +-14 degrees


def case(name):
    if name in _CASES:
        return _CASES[name]
    G = GC.cases()
    if name == "room_table_c16":                                                    # the golden room from ROOM_EYES[0] with the table of the sibling passes
        c = Case(name, G["room_a_c16"], ["table"], [0], [MC.TABLE_AT(3.6, 2.6)])       # (nearer the eye than the siblings' pose: it covers a twentieth of the view)
    elif name == "stride_c296":
        c = Case(name, G["box_stride_c296"], ["ico"], [0], [_stride_instance(G["box_stride_c296"])])
    else:
        kind, eye, cc = name.rsplit("_", 2)
        occ, inst, poses, deg = arrangement(kind, EYES[eye])
        c = Case(name, G["box_%s_%s" % (eye, cc)], occ, inst, poses, degenerate=deg)
    _CASES[name] = c
    return c


MUTANT_CASES = {"w_not_transposed": "box_graze_c8", "not_normalised": "box_centre_c8", "mirror_flipped": "mirror_graze_c17", "object_space_pos": "ico_centre_c8",
                "unbounded": "cut_graze_c17", "last_wins": "inter_centre_c17", "inst_off_by_one": "twice_centre_c8", "tri_no_plus_1": "ico_graze_c17",
                "uv_not_zero": "box_centre_c17", "uv_da_kept": "box_graze_c17"}
