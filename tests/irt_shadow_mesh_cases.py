"""Cases of the mesh-shadow pass (include/texir_hip.h texir_irt_shadow_mesh, csrc/irtshadowmesh.hip): the float64 reference, the check of a result against
it, a float32 restatement of the rule with the mutants the check must reject, and the seeded cases.  Shared by test_irt_shadow_mesh_ref_cpu.py (no GPU) and
test_gpu_irt_shadow_mesh.py; no tests here.  Rays, candidate lists, radiance intervals and the direction chain come from trace_cases / spec_cases, the
classes of an occlusion query from occlusion_cases, the way outcomes and sets combine from irt_shadow_cases; none of them is changed.  KF = 4, U = 2^-24 and
TINY are texture_cases'; every margin is the header's ROUNDING BOUND times KF, fixed before any GPU run; nothing is taken from a kernel's output.

THE REFERENCE is trace_cases.IrtRef's per-sample outcomes (every admissible direction variant, every admissible closest-hit candidate with its distance
t_s +- bound_t and its radiance interval, the zero outcome where a miss or the cut t > 1e-4 admits it), each extended per instance j:
  object-space ray        o' in the rule's float32 sequence in numpy (a fixed value on any IEEE machine), d' = W d in float64 with the bound
                          |W| e + KF 3 u |W| |d| of the header
  instance j against candidate c   trace_cases.RayRef over the OCCLUDER's triangles along (o', d' +- bound), classified by occlusion_cases.classify_rayref:
                          certainly BLOCKED: certainly occluded inside (0, t_s - bound_t);  certainly CLEAR: certainly visible inside (0, t_s + bound_t);
                          else uncertain
  set m against candidate c, the interval of an outcome, the hull over outcomes, the widening of a texel: as irt_shadow_cases has them.
stats (prefilter on) must lie between certain counts and certain plus uncertain counts over the LIST: [0] samples whose object-space ray meets some
instance's box -- certainly: the exact line meets the box padded by HALF the header's P for every direction inside the bound (the kernel's own roundings
are a fraction of that) and the far plane lies ahead along every axis that may be the dominant one; possibly: it meets the box padded by twice P for some
direction inside the bound and the far plane lies ahead along some axis that may be the dominant one; [1] occluder queries = per
instance, met and an accepted scene hit; [2] blocked samples.
CAPS (from the reference alone, asserted in test_irt_shadow_mesh_ref_cpu.py): no ray overflows a candidate list; at most CAP_MULTI = 2 % of the samples that
may meet a box are uncertain in any of this.
"""
import math

import numpy as np

import irt_shadow_cases as SH
import occlusion_cases as OC
import spec_cases as SC  # noqa: F401  (the direction chain behind IrtRef)
import trace_cases as TC
from texture_cases import K as KF, TINY, U

F32, F64 = np.float32, np.float64
CAP_MULTI = TC.CAP_MULTI
SENTINEL = 7.0
MAX_INST = MAX_SETS = 8
BOX_PAD = 2.0 ** -18                # the header's P per unit of (rb + |o'|_inf)


# ---- meshes (object space) -------------------------------------------------------------------------------------------------------------------------------------

def occ_geo(name, verts, tris):
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    return TC.Geo(name, np.asarray(verts, F32), tris, np.zeros((3 * len(tris), 2), F32), np.zeros((1, 1, 3), F32))


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = [(a, b, c) for a, b, c, d in q] + [(a, c, d) for a, b, c, d in q]
    return v, np.array(t, np.int32)


def join(parts):
    vs, ts, n = [], [], 0
    for v, t in parts:
        vs.append(v)
        ts.append(t + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def icosphere(levels=1, r=1.0):
    p = (1 + math.sqrt(5)) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, F64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, t2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            t2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = t2
    return np.array(v) * r, np.array(t, np.int32)


def uv_sphere(n_lon=32, n_lat=32, r=(1.0, 1.0, 1.0)):
    """2 n_lon (n_lat - 1) triangles: 1984 at 32 x 32"""
    v = [(0.0, 1.0, 0.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * (j + 0.5 * (i & 1)) / n_lon
            v.append((math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    t = [(0, ring(1, j + 1), ring(1, j)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            t += [(ring(i, j), ring(i, j + 1), ring(i + 1, j)), (ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j))]
    last = len(v) - 1
    t += [(last, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)) for j in range(n_lon)]
    return np.array(v) * np.asarray(r, F64), np.array(t, np.int32)


_OCC = {}


def occluder(name):
    """the occluders of the cases, in object space"""
    if name not in _OCC:
        if name == "tri":
            g = occ_geo(name, [[-1.5, 0.0, -1.0], [1.5, 0.0, -1.0], [0.0, 0.0, 2.0]], [[0, 1, 2]])
        elif name == "cube":
            g = occ_geo(name, *box_mesh([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]))
        elif name == "ico":
            g = occ_geo(name, *icosphere(1, 0.5))
        elif name == "table":                                                      # a top and four legs: five boxes, 60 triangles, standing on y = 0
            legs = [box_mesh([x - 0.05, 0.0, z - 0.05], [x + 0.05, 0.7, z + 0.05]) for x in (-0.6, 0.6) for z in (-0.35, 0.35)]
            g = occ_geo(name, *join([box_mesh([-0.7, 0.7, -0.45], [0.7, 0.76, 0.45])] + legs))
        elif name == "person":                                                     # a 1984-triangle ellipsoid 1.7 tall, standing on y = 0
            v, t = uv_sphere(32, 32, (0.3, 0.85, 0.22))
            g = occ_geo(name, v + np.array([0.0, 0.85, 0.0]), t)
        else:
            raise KeyError(name)
        _OCC[name] = g
    return _OCC[name]


N_TRIS = {"tri": 1, "cube": 12, "ico": 80, "table": 60, "person": 1984}


def pose(translate=(0, 0, 0), axis=(0, 1, 0), deg=0.0, scale=1.0):
    """object-to-world [3,4] float64"""
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + s * Kx + (1 - c) * Kx @ Kx
    return np.concatenate([R * np.asarray(scale, F64), np.asarray(translate, F64)[:, None]], 1)


def to_world_to_object(poses):
    from texir_code_amd import scene as S
    return S.world_to_object(np.asarray(poses, F64).reshape(-1, 3, 4))


# ---- the rule's float32 pieces ------------------------------------------------------------------------------------------------------------------------------------

def point_f32(W, x):
    """o' [R,3] float32: the header's sequence; W [12] float32, x [R,3] float32"""
    W, x = np.asarray(W, F32).reshape(3, 4), np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return np.stack([((W[r, 0] * x[:, 0] + W[r, 1] * x[:, 1]) + W[r, 2] * x[:, 2]) + W[r, 3] for r in range(3)], 1).astype(F32)


def dir_f32(W, d):
    W, d = np.asarray(W, F32).reshape(3, 4), np.asarray(d, F32)
    with np.errstate(all="ignore"):
        return np.stack([(W[r, 0] * d[:, 0] + W[r, 1] * d[:, 1]) + W[r, 2] * d[:, 2] for r in range(3)], 1).astype(F32)


def box_classes(lo, hi, o, d, e):
    """the prefilter's answer for the line (o, d +- e), o [R,3] exact, d, e [R,3] float64 (e: KF included) -> (certainly met, possibly met) [R]"""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    rb = max(np.abs(lo).max(), np.abs(hi).max())
    P = BOX_PAD * (rb + np.abs(o).max(1)) + 1e-30
    ad = np.abs(d)
    live = np.isfinite(d).all(1) & (ad.max(1) > 0)

    def run(l3, h3, sure):
        tn, tf = np.full(len(o), -np.inf), np.full(len(o), np.inf)
        okay = np.ones(len(o), bool)
        for r in range(3):
            l, h = (l3[r] if np.ndim(l3[r]) else np.full(len(o), l3[r])), (h3[r] if np.ndim(h3[r]) else np.full(len(o), h3[r]))
            flat = ad[:, r] <= e[:, r]
            inside = (o[:, r] > l) & (o[:, r] < h) if sure else (o[:, r] >= l) & (o[:, r] <= h)
            with np.errstate(all="ignore"):
                cs = [(p - o[:, r]) / dd for p in (l, h) for dd in (d[:, r] - e[:, r], d[:, r] + e[:, r])]
                a = [np.minimum(cs[0], cs[2]), np.minimum(cs[1], cs[3])]               # the near plane under either direction, the far plane alike
                n_lo, n_hi = np.minimum(a[0], a[1]), np.maximum(a[0], a[1])
                b = [np.maximum(cs[0], cs[2]), np.maximum(cs[1], cs[3])]
                f_lo, f_hi = np.minimum(b[0], b[1]), np.maximum(b[0], b[1])
            w = 2.0 ** -40 if sure else 2.0 ** -20
            if sure:
                n, f = n_hi + np.abs(n_hi) * w, f_lo - np.abs(f_lo) * w
                okay &= np.where(flat, inside, True)
                tn, tf = np.where(flat, tn, np.maximum(tn, n)), np.where(flat, tf, np.minimum(tf, f))
            else:
                n, f = n_lo - np.abs(n_lo) * w, f_hi + np.abs(f_hi) * w
                tn, tf = np.where(flat, tn, np.maximum(tn, n)), np.where(flat, tf, np.minimum(tf, f))
        # the far plane ahead along an axis that may be the dominant one
        dom = ad + e >= (ad - e).max(1, keepdims=True)
        ahead = np.where(d > 0, np.stack([h3[r] - o[:, r] for r in range(3)], 1) > 0, np.stack([o[:, r] - l3[r] for r in range(3)], 1) > 0)
        sign_sure = ad > e
        if sure:
            fwd = (np.where(dom, ahead & sign_sure, True)).all(1)
            return okay & fwd & (tn < tf)
        fwd = (dom & (ahead | ~sign_sure)).any(1)
        return fwd & ~(tn > tf)
    # certainly: half the kernel's pad (its own roundings are a fraction of that); possibly: twice the pad
    yes = live & run([lo[r] - 0.5 * P for r in range(3)], [hi[r] + 0.5 * P for r in range(3)], True)
    maybe = ~live | run([lo[r] - 2 * P for r in range(3)], [hi[r] + 2 * P for r in range(3)], False)
    return yes, maybe | yes


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------

class Case:
    """pos, nrm [Nt,3], shift [Nt,2] f32 of the whole grid; ids: the listed texels; occ: names of the Q occluders; inst: occluder index per instance of the
    BUFFER, of which the first K are the call's; poses [Kbuf,3,4] object-to-world; sets: M masks"""

    def __init__(self, name, geo, pos, nrm, shift, ids, N, mode, occ, inst, poses, sets, K=None):
        self.name, self.geo = "mesh:" + name, geo                                 # (irt_shadow_cases.traced caches by name: its own cases have these names too)
        self.pos, self.nrm = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.Nt = self.pos.shape[0]
        self.shift = np.ascontiguousarray(shift, F32).reshape(self.Nt, 2)
        self.ids = np.ascontiguousarray(ids, np.int32)
        self.N, self.mode = int(N), mode
        self.occ = list(occ)
        self.inst_buf = [int(i) for i in inst]
        self.poses_buf = np.asarray(poses, F64).reshape(-1, 3, 4)
        self.w2o_buf = to_world_to_object(self.poses_buf) if len(self.inst_buf) else np.zeros((0, 12), F32)
        self.K = len(self.inst_buf) if K is None else int(K)
        self.inst, self.poses, self.w2o = self.inst_buf[:self.K], self.poses_buf[:self.K], self.w2o_buf[:self.K]
        self.sets = [int(s) & 0xFFFFFFFF for s in sets]
        self.M = len(self.sets)
        self.parts = TC.n_parts(self.N, "group")
        self._ref = None

    def masks(self):
        return [s & ((1 << self.K) - 1) for s in self.sets]

    def geos(self):
        return [occluder(n) for n in self.occ]

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref


class Ref:
    def __init__(self, case):
        self.case = c = case
        L = np.unique(c.ids.astype(np.int64))
        self.tex = L
        self.row_of = {int(t): i for i, t in enumerate(L)}
        N, P = c.N, len(L)
        irt = self.irt = TC.IrtRef(c.geo, c.pos[L], c.nrm[L], c.shift[L], N, c.mode)
        rays, si, vi = irt.rays, irt.sample_of, irt.variant_of
        names = ("d0", "d1", "d2")
        d = np.stack([irt.dref.val[k][vi, si] for k in names], 1)
        bd = np.stack([irt.dref.bnd[k][vi, si] for k in names], 1)               # KF included
        x32 = c.pos[L][si // N]
        n = c.nrm.astype(F64)[L][si // N]
        nd = (n * d).sum(1)
        en = (np.abs(n) * bd).sum(1) + KF * (3 * U * (np.abs(n) * np.abs(d)).sum(1) + 3 * TINY)
        f, f_lo, f_hi = np.clip(nd, 0, 1), np.clip(nd - en, 0, 1), np.clip(nd + en, 0, 1)
        lo, hi, val, ok = rays.outcomes()                                        # [R, C + 1, 3]; the last slot is the zero outcome
        prod = [lo * f_lo[:, None, None], lo * f_hi[:, None, None], hi * f_lo[:, None, None], hi * f_hi[:, None, None]]
        o_lo, o_hi = np.minimum.reduce(prod), np.maximum.reduce(prod)
        o_val = val * f[:, None, None]
        R, C1 = ok.shape
        C = C1 - 1
        with np.errstate(invalid="ignore"):
            t_lo, t_hi, t_s = rays.t - rays.bt, rays.t + rays.bt, rays.t          # [R, C]
        Kb = c.K
        blocked = np.zeros((Kb, R, C), bool)
        clear = np.ones((Kb, R, C), bool)
        front64 = np.zeros((Kb, R, C), bool)
        m_yes, m_maybe = np.zeros((Kb, R), bool), np.zeros((Kb, R), bool)
        self.overflow = int(rays.overflow.sum())
        self.box_pin_fails = 0
        geos = c.geos()
        for k in range(Kb):
            g = geos[c.inst[k]]
            W = c.w2o[k].astype(F64).reshape(3, 4)
            o32 = point_f32(c.w2o[k], x32).astype(F64)
            d_o = d @ W[:, :3].T
            bd_o = bd @ np.abs(W[:, :3]).T + KF * (3 * U * (np.abs(d) @ np.abs(W[:, :3]).T) + 3 * TINY)
            tri = g.verts[g.tris.reshape(-1)]
            m_yes[k], m_maybe[k] = box_classes(tri.min(0), tri.max(0), o32, d_o, bd_o)
            sel = np.nonzero(m_maybe[k])[0]                                       # (a ray that certainly misses the box meets no triangle inside it)
            rr = TC.RayRef(g, o32[sel], d_o[sel], bd_o[sel])
            self.overflow += int(rr.overflow.sum())
            for cc in range(C):
                occ_, _ = OC.classify_rayref(rr, t_lo[sel, cc][:, None])
                _, vis = OC.classify_rayref(rr, t_hi[sel, cc][:, None])
                blocked[k][sel, cc] = occ_
                clear[k][sel, cc] = vis
                with np.errstate(invalid="ignore"):
                    front64[k][sel, cc] = (rr.has & (rr.c["robust"] > 0) & (rr.t > 0) & (rr.t < t_s[sel, cc][:, None])).any(1)
            # certainly met by a triangle: then certainly by the box (the pin of box_classes against the triangle lists)
            hit_sure, _ = OC.classify_rayref(rr, np.inf)
            self.box_pin_fails += int((hit_sure & ~m_yes[k][sel] & (np.abs(d_o[sel]) > 64 * bd_o[sel]).all(1)).sum())
        cand_ok = ok[:, :C]

        def per_sample(x_, fn, init):
            out = np.full((P * N,) + x_.shape[1:], init, x_.dtype)
            fn.at(out, si, x_)
            return out.reshape((P, N) + x_.shape[1:])
        base = np.nonzero(vi == 0)[0]
        first = ok[base].argmax(1)
        self.lo, self.hi, self.mid = [], [], []
        for mask in c.masks():
            ks = [k for k in range(Kb) if mask >> k & 1]
            bl = blocked[ks].any(0) if ks else np.zeros((R, C), bool)
            cl = clear[ks].all(0) if ks else np.ones((R, C), bool)
            fr = front64[ks].any(0) if ks else np.zeros((R, C), bool)
            z = np.zeros((R, 1), bool)
            bl3, cl3 = np.concatenate([bl, z], 1)[..., None], np.concatenate([cl, ~z], 1)[..., None]
            s_lo = np.where(bl3, o_lo, np.where(cl3, 0.0, np.minimum(o_lo, 0.0)))
            s_hi = np.where(bl3, o_hi, np.where(cl3, 0.0, np.maximum(o_hi, 0.0)))
            r_lo = np.where(ok[..., None], s_lo, np.inf).min(1)
            r_hi = np.where(ok[..., None], s_hi, -np.inf).max(1)
            self.lo.append(per_sample(r_lo, np.minimum, np.inf))
            self.hi.append(per_sample(r_hi, np.maximum, -np.inf))
            v = np.where(np.concatenate([fr, z], 1)[..., None], o_val, 0.0)
            mid = np.zeros((P * N, 3))
            mid[si[base]] = v[base, first]
            self.mid.append(mid.reshape(P, N, 3))
        # counts per sample
        acc_yes = ~ok[:, C] & cand_ok.any(1)
        acc_maybe = cand_ok.any(1)
        meet_yes = m_yes.any(0) if Kb else np.zeros(R, bool)
        meet_maybe = m_maybe.any(0) if Kb else np.zeros(R, bool)
        any_bl = blocked.any(0) if Kb else np.zeros((R, C), bool)
        all_cl = clear.all(0) if Kb else np.ones((R, C), bool)
        blk_yes = ~ok[:, C] & np.where(cand_ok, any_bl, True).all(1) & cand_ok.any(1)
        blk_maybe = (cand_ok & ~all_cl).any(1)
        unc_ray = (meet_maybe & ~meet_yes) | (m_maybe & ~m_yes).any(0) | (meet_maybe & (cand_ok & ~any_bl & ~all_cl).any(1)) if Kb else np.zeros(R, bool)
        self.meet_yes = per_sample(meet_yes, np.logical_and, True)               # [P, N]: every variant
        self.meet_maybe = per_sample(meet_maybe, np.logical_or, False)
        self.q_yes = sum(per_sample(m_yes[k] & acc_yes, np.logical_and, True).astype(np.int64) for k in range(Kb)) if Kb else np.zeros((P, N), np.int64)
        self.q_maybe = sum(per_sample(m_maybe[k] & acc_maybe, np.logical_or, False).astype(np.int64) for k in range(Kb)) if Kb else np.zeros((P, N), np.int64)
        self.blk_yes = per_sample(blk_yes, np.logical_and, True)
        self.blk_maybe = per_sample(blk_maybe, np.logical_or, False)
        self.uncertain = per_sample(unc_ray, np.logical_or, False)
        self.scale = 2.0 * math.pi / N

    def caps(self):
        """(rays that overflow a list, share of the samples that may meet a box in which anything is uncertain)"""
        return self.overflow, float(self.uncertain.sum()) / max(int(self.meet_maybe.sum()), 1)

    def counts(self):
        """over the LIST (a duplicate counts again): [(lo, hi)] of stats[0], [1], [2]"""
        rows = np.array([self.row_of[int(t)] for t in self.case.ids], np.int64)
        g = lambda a: int(a[rows].sum())
        return [(g(self.meet_yes), g(self.meet_maybe)), (g(self.q_yes), g(self.q_maybe)), (g(self.blk_yes), g(self.blk_maybe))]

    def all_blocked(self, m):
        """[P] bool: every sample of the texel is, for set m, either certainly without an accepted hit or certainly blocked, and at least one is blocked --
        the texels on which lost[m] must equal irt_generate bit for bit"""
        irt = self.irt
        lo, hi = self.lo[m], self.hi[m]
        same = ((lo == irt.lo) & (hi == irt.hi)).all(2)
        sure = irt.n_out == 1
        return (same & sure).all(1) & (np.abs(self.mid[m]).sum((1, 2)) > 0)

    def summary(self):
        over, unc = self.caps()
        return {"texels": len(self.tex), "samples": int(self.meet_maybe.size), "may_meet": int(self.meet_maybe.sum()), "uncertain_share": unc, "overflow": over,
                "counts": self.counts(), "lost_share": [float((np.abs(m_).sum((1, 2)) > 0).mean()) for m_ in self.mid]}


RATIOS = {}


def check(case, lost, stats=None, sentinel=None, what=""):
    """lost [M, Nt, 3]: every listed texel of every set inside its interval, unlisted texels keep `sentinel`, stats inside its counts -> the worst
    error / bound; raises AssertionError naming what fails"""
    ref = case.ref()
    lost = np.asarray(lost, F64).reshape(case.M, case.Nt, 3)
    fails, worst = [], 0.0
    got_all = lost[:, ref.tex]
    if not np.isfinite(got_all).all():
        fails.append("non-finite values")
    nr = TC.n_acc(case.N, "group", case.parts)
    for m in range(case.M):
        lo_s, hi_s = ref.lo[m], ref.hi[m]
        LO, HI = lo_s.sum(1), hi_s.sum(1)
        mag = np.maximum(np.abs(lo_s), np.abs(hi_s)).sum(1)
        acc = KF * (nr * U * mag + (nr + 4) * TINY)
        lo, hi = ref.scale * (LO - acc), ref.scale * (HI + acc)
        mid = ref.scale * ref.mid[m].sum(1)
        got = got_all[m]
        zero = (LO == 0) & (HI == 0) & (mag == 0)
        if (got[zero] != 0).any() or np.signbit(got[zero]).any():
            fails.append("set %d: %d values of texels no sample of which can be blocked are not +0" % (m, int((got[zero] != 0).sum())))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(got >= mid, np.where(got == mid, 0.0, (got - mid) / (hi - mid)), (mid - got) / (mid - lo))
        ratio = np.where(zero, 0.0, ratio)
        bad = ~(ratio <= 1.0)
        for i, ch in np.argwhere(bad)[:6]:
            fails.append("set %d texel %d channel %d: %.9g outside [%.9g, %.9g] (reference %.9g)" % (m, ref.tex[i], ch, got[i, ch], lo[i, ch], hi[i, ch], mid[i, ch]))
        if bad.sum() > 6:
            fails.append("... set %d: %d values outside in all" % (m, int(bad.sum())))
        if ratio.size and not bad.any():
            worst = max(worst, float(ratio.max()))
    if sentinel is not None:
        un = np.setdiff1d(np.arange(case.Nt), ref.tex)
        if un.size and not (lost[:, un] == sentinel).all():
            fails.append("unlisted texels were written")
    if stats is not None:
        s = [int(v) for v in np.asarray(stats).reshape(-1)[:3]]
        for i, (a, b) in enumerate(ref.counts()):
            if not a <= s[i] <= b:
                fails.append("stats[%d] = %d outside [%d, %d]" % (i, s[i], a, b))
    print("error/bound irt_shadow_mesh %-36s %s" % (case.name + " " + what, "rejected" if fails else "%.4f" % worst))
    if fails:
        raise AssertionError("%s %s:\n%s" % (case.name, what, "\n".join(fails)))
    RATIOS[case.name] = max(RATIOS.get(case.name, 0.0), worst)
    return worst


# ---- float32 restatement of the rule (CPU), op by op, with the mutants the check must reject ------------------------------------------------------------------------

MUTANTS = ("far_ignored", "transposed", "no_translation", "translated_dir", "add_missed", "sum_sets", "high_bits", "world_space")


def box_f32(lo, hi, o, d):
    """the header's PREFILTER in float32, operation by operation -> [R] bool"""
    lo, hi, o, d = np.asarray(lo, F32), np.asarray(hi, F32), np.asarray(o, F32), np.asarray(d, F32)
    with np.errstate(all="ignore"):
        a = np.abs(d)
        am = a.max(1)
        free = ~((am > 0) & (am < np.inf))
        rb = max(np.abs(lo).max(), np.abs(hi).max())
        P = (F32(BOX_PAD) * (rb + np.abs(o).max(1))).astype(F32) + F32(1e-30)
        l3, h3 = (lo[None] - P[:, None]).astype(F32), (hi[None] + P[:, None]).astype(F32)
        kz = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
        rr = np.arange(len(o))
        fwd = np.where(d[rr, kz] > 0, h3[rr, kz] > o[rr, kz], l3[rr, kz] < o[rr, kz])
        tn, tf = np.full(len(o), -np.inf, F32), np.full(len(o), np.inf, F32)
        okay = fwd.copy()
        w = F32(2.0 ** -21)
        for r in range(3):
            flat = d[:, r] == 0
            okay &= np.where(flat, (o[:, r] >= l3[:, r]) & (o[:, r] <= h3[:, r]), True)
            inv = (F32(1) / d[:, r]).astype(F32)                                   # (the kernel's reciprocal is within 1 ulp of this one)
            x, y = ((l3[:, r] - o[:, r]) * inv).astype(F32), ((h3[:, r] - o[:, r]) * inv).astype(F32)
            n, f = np.where(x < y, x, y), np.where(x < y, y, x)
            n2, f2 = (n - np.abs(n) * w).astype(F32), (f + np.abs(f) * w).astype(F32)
            tn = np.where(~flat & (n2 > tn), n2, tn)
            tf = np.where(~flat & (f2 < tf), f2, tf)
        return free | (okay & ~(tn > tf))


_LEAF = {}


def shadow_mesh_f32(case, mut=None, sentinel=SENTINEL, prefilter=True):
    """-> (lost [M,Nt,3] f32, stats [3]); unlisted texels hold the sentinel"""
    c = case
    L, d, t, pid, rad = SH.traced(c)
    P, N = len(L), c.N
    x, dr = np.repeat(c.pos[L], N, 0), d.reshape(-1, 3).astype(F32)
    accepted = np.isfinite(t) & (t > F32(1e-4)) & (pid >= 0)
    n_inst = len(c.inst_buf) if mut == "high_bits" else c.K
    geos = c.geos()
    met, front = np.zeros((n_inst, P * N), bool), np.zeros((n_inst, P * N), bool)
    for k in range(n_inst):
        g = geos[c.inst_buf[k]]
        W = c.w2o_buf[k].copy().reshape(3, 4)
        if mut == "transposed":
            W[:, :3] = W[:, :3].T.copy()
        if mut == "no_translation":
            W[:, 3] = 0
        if mut == "world_space":
            W = np.eye(3, 4, dtype=F32)
        if not np.isfinite(W).all():
            continue
        o, dd = point_f32(W, x), dir_f32(W, dr)
        if mut == "translated_dir":
            dd = (dd + W[None, :, 3]).astype(F32)
        tri = g.verts[g.tris.reshape(-1)]
        met[k] = box_f32(tri.min(0), tri.max(0), o, dd) if prefilter else True
        key = (c.name, k, mut if mut in ("transposed", "no_translation", "world_space", "translated_dir") else None)
        if key not in _LEAF:
            _LEAF[key] = OC.leaf_f32(g, o, dd)
        inside, tt = _LEAF[key]
        with np.errstate(invalid="ignore"):
            far = np.full_like(t, np.inf) if mut == "far_ignored" else t
            hit = (inside & (tt > 0) & (tt < far[:, None])).any(1)
        assert not (hit & ~met[k]).any(), "the prefilter rejects a ray the leaf test accepts"
        front[k] = hit
    take = np.ones(P * N, bool) if mut == "add_missed" else accepted
    Lr = np.where(accepted[:, None], rad, F32(1)).astype(F32)                    # (add_missed: a ray that leaves the scene carries radiance 1)
    out = np.full((c.M, c.Nt, 3), sentinel, F32)
    for m, mask in enumerate(c.sets if mut == "high_bits" else c.masks()):
        ks = [k for k in range(n_inst) if mask >> k & 1]
        if mut == "sum_sets":
            w = front[ks].sum(0).astype(F32) if ks else np.zeros(P * N, F32)
        else:
            w = (front[ks].any(0) if ks else np.zeros(P * N, bool)).astype(F32)
        terms = (Lr * (w * take)[:, None]).astype(F32)
        out[m, L] = TC.estimator_f32(c.nrm[L], d, terms.reshape(P, N, 3), False, "group", c.parts)
    mult = np.bincount(np.searchsorted(L, c.ids.astype(np.int64)), minlength=P)
    anymet = met.any(0).reshape(P, N) if n_inst else np.zeros((P, N), bool)
    queries = (met & accepted[None]).sum(0).reshape(P, N) if n_inst else np.zeros((P, N), np.int64)
    anyfront = (front.any(0) & accepted).reshape(P, N) if n_inst else np.zeros((P, N), bool)
    return out, np.array([(anymet * mult[:, None]).sum(), (queries * mult[:, None]).sum(), (anyfront * mult[:, None]).sum()], np.int64)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------------------------

# the box is [0, 8] x [0, 3] x [0, 6] and so, within half a centimetre, is the room; texels sit 0.01 inside their faces
TABLE_AT = lambda x=4.0, z=3.0, deg=20.0: pose((x, 0.0, z), (0, 1, 0), deg)
ICO_AT = lambda x=4.0, y=1.25, z=3.0, deg=35.0, s=1.0: pose((x, y, z), (1, 2, 3), deg, s)
BELOW = lambda: pose((-3.0, -3.0, -3.0))                                           # beyond the corner x, y, z < 0, axes parallel to the world's


def eight_instances():
    """(inst, poses) over the occluders (ico, cube): overlapping pairs, a scaled and a sheared one, one under the floor"""
    shear = pose((6.0, 1.0, 4.5), (0, 0, 1), 15.0)
    shear[0, 1] += 0.4
    return [0, 0, 1, 1, 0, 1, 0, 1], np.stack([ICO_AT(2.0, 1.0, 2.0), ICO_AT(2.4, 1.2, 2.2, 80.0), pose((5.5, 0.5, 1.5), (0, 1, 0), 30.0), shear, ICO_AT(4.0, 2.2, 4.0, 10.0, 1.5),
                                               pose((1.0, 2.0, 5.0), (1, 0, 0), 45.0, 0.5), ICO_AT(6.5, 0.3, 2.5, 0.0, 0.4), BELOW()])


_CASES = {}


def enclosing_cube(geo_name="box"):
    """a closed box around a patch of floor texels that cuts through the floor: every ray of an enclosed texel meets it from inside before anything else"""
    return pose((4.0, 0.0, 3.0), (0, 1, 0), 0.0, (3.0, 1.0, 2.5))                  # x in [2.5, 5.5], y in [-0.5, 0.5], z in [1.75, 4.25]


def enclosed_ids(scene, n=None):
    _, gb = TC.golden_geo(scene)
    p, nn = gb["pos"].reshape(-1, 3), gb["nrm"].reshape(-1, 3)
    v = np.argwhere((gb["valid"].reshape(-1) > 0) & (nn[:, 1] > 0.9) & (np.abs(p[:, 0] - 4.0) < 1.2) & (np.abs(p[:, 2] - 3.0) < 1.0) & (p[:, 1] < 0.3))[:, 0]
    return v if n is None else v[:n]


def case(name):
    if name in _CASES:
        return _CASES[name]
    scene = "room" if name.startswith("room") else "box"
    geo, gb = TC.golden_geo(scene)
    pos, nrm, shift = gb["pos"].reshape(-1, 3), gb["nrm"].reshape(-1, 3), gb["shift"].reshape(-1, 2)
    spread, floor = (lambda n: SH.spread(scene, n)), SH.floor_ids
    mk = lambda ids, N, mode, occ, inst, poses, sets, K=None, g=geo: Case(name, g, pos, nrm, shift, ids, N, mode, occ, inst, poses, sets, K)
    big_tri = pose((4.0, 1.5, 3.0), (0, 0, 1), 10.0, 2.0)
    if name == "box_one":                                                          # one texel, one sample, one triangle over it, two sets
        c = mk(floor()[80:81], 1, "uniform", ["tri"], [0], [pose((0, 0.4, 0), scale=50.0)], [1, 0])
    elif name == "box_tri":                                                        # 63 texels, N = 2
        c = mk(spread(63), 2, "uniform", ["tri"], [0], [big_tri], [1])
    elif name == "box_cube":                                                       # 64 texels, N = 63 (no power of two: one part, natural order)
        c = mk(spread(64), 63, "uniform", ["cube"], [0], [pose((3.0, 1.0, 2.0), (1, 1, 0), 30.0, 1.5)], [1])
    elif name == "box_ico_twice":                                                  # 65 texels, one handle twice, overlapping: the sets {0}, {1}, {0, 1}
        c = mk(floor(65), 64, "uniform", ["ico"], [0, 0], [ICO_AT(), ICO_AT(4.3, 1.4, 3.2, 70.0)], [1, 2, 3])
    elif name == "box_table":                                                      # 130 texels (two waves and two lanes), N = 65
        c = mk(spread(130), 65, "uniform", ["table"], [0], [TABLE_AT()], [1])
    elif name == "box_table_small":                                                # the same at a size the CPU restatement and its mutants afford
        c = mk(spread(40), 64, "uniform", ["table"], [0], [TABLE_AT()], [1])
    elif name == "room_two":                                                       # Q = 2, N = 100
        c = mk(spread(130), 100, "uniform", ["table", "ico"], [0, 1], [TABLE_AT(3.0, 2.5), ICO_AT(5.5, 1.0, 3.5)], [1, 2])
    elif name == "room_small":
        c = mk(spread(10), 64, "uniform", ["table", "ico"], [0, 1], [TABLE_AT(3.0, 2.5), ICO_AT(5.5, 1.0, 3.5)], [1, 2, 3])
    elif name == "room_person":                                                    # the 1984-triangle object, the cosine mode, N = 128: 16 parts
        c = mk(spread(65), 128, "cosine", ["person"], [0], [pose((4.0, 0.0, 3.0), (0, 1, 0), 40.0)], [1])
    elif name == "box_person":
        c = mk(floor(64), 64, "uniform", ["person"], [0], [pose((4.0, 0.0, 3.0), (0, 1, 0), 40.0)], [1])
    elif name == "box_eight":                                                      # K = 8, M = 8, N = 512: 32 parts; every kind of mask
        inst, poses = eight_instances()
        c = mk(spread(64), 512, "uniform", ["ico", "cube"], inst, poses, [1, 2, 3, 0, 0xFFFFFF00 | 8, 0xFF, 0x20, 0x40 | 0x80])
    elif name == "box_eight_small":
        inst, poses = eight_instances()
        c = mk(spread(30), 64, "uniform", ["ico", "cube"], inst, poses, [1, 2, 3, 0, 0xFFFFFF00 | 8, 0xFF, 0x20, 0x40 | 0x80])
    elif name == "box_highbits":                                                   # K = 1 of a buffer of two: bit 1 names no instance of the call
        c = mk(spread(63), 64, "uniform", ["ico", "table"], [0, 1], [ICO_AT(), TABLE_AT()], [1, 2, 3], K=1)
    elif name == "box_none":                                                       # K = 0
        c = mk(spread(65), 64, "uniform", [], [], np.zeros((0, 3, 4)), [1])
    elif name == "box_below":                                                      # beyond the corner under the floor, floor texels: along the dominant axis the far
        # plane lies behind, or the line reaches the box's x or z range only ahead, where y has risen: the box test passes for no ray
        c = mk(floor(65), 64, "uniform", ["cube", "ico"], [0, 1], [BELOW(), pose((-2.0, -4.0, -2.5))], [1, 2, 3])
    elif name == "box_behind_wall":                                                # behind the wall x = 0: met by rays, never in front of the scene's hit
        c = mk(spread(65), 64, "uniform", ["ico"], [0], [ICO_AT(-1.5, 1.5, 3.0)], [1])
    elif name == "box_open_top":                                                   # above the open top: met only by rays that leave the scene
        c = mk(floor(65), 64, "uniform", ["ico", "cube"], [0, 1], [ICO_AT(4.0, 6.0, 3.0, 35.0, 3.0), pose((4.0, 1.25, 3.0), (0, 1, 0), 20.0)], [1, 2], g=SH.box_open())
    elif name == "box_enclosed":                                                   # every listed texel inside a closed box that cuts through the floor
        c = mk(enclosed_ids("box"), 64, "uniform", ["cube", "ico"], [0, 1], [enclosing_cube(), ICO_AT(-20.0, 30.0, -20.0)], [1, 2, 3])
    elif name == "room_enclosed":
        c = mk(enclosed_ids("room", 130), 64, "uniform", ["cube"], [0], [enclosing_cube()], [1])
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


GPU_CASES = ("box_one", "box_tri", "box_cube", "box_ico_twice", "box_table", "box_table_small", "room_two", "room_small", "room_person", "box_person", "box_eight",
             "box_eight_small", "box_highbits", "box_none", "box_below", "box_behind_wall", "box_open_top", "box_enclosed", "room_enclosed")
CPU_CASES = ("box_one", "box_tri", "box_cube", "box_ico_twice", "box_table_small", "room_small", "box_eight_small", "box_highbits", "box_none", "box_below",
             "box_behind_wall", "box_open_top", "box_enclosed")
# where each mutant must be rejected
MUTANT_CASES = {"far_ignored": "box_behind_wall", "transposed": "box_cube", "no_translation": "box_table_small", "translated_dir": "box_table_small",
                "add_missed": "box_open_top", "sum_sets": "box_ico_twice", "high_bits": "box_highbits", "world_space": "box_table_small"}
