"""Float64 reference of the inserted-emitter rule (include/texir_hip.h, texir_irt_lights) per (texel, light, sample), the check of a result against it, the
float32 restatement of the kernel's arithmetic with its mutants, and the seeded cases.  Shared by test_irt_lights_ref_cpu.py (no GPU) and
test_gpu_irt_lights.py; no tests here.  K = 4, U = 2^-24 and TINY are texture_cases'; every margin below is the header's ROUNDING BOUND times K, nothing is
taken from a kernel's output.

THE SAMPLE POINT (s0, s1) is restated in float32 (ham0, ham1, shift_wrap_clamp of csrc/device_common.h are IEEE additions, comparisons and exact scalings:
the same bits on any IEEE machine) and held in float64 from there on, as the header's bound does.

PER (TEXEL, LIGHT, SAMPLE), from the float32 inputs held in float64:
  geometry   y, m, d, dd, nd, md and g = nd md / dd^2 exactly, with the header's bounds e (of d), f (of m), |dnd|, |dmd| and |dg| = eg.  The sphere's sqrt is
             correctly rounded, its sinf / cosf are taken at 4 ulp, as the header states.
  sign       nd > 0 and md > 0 are CERTAINLY TRUE beyond K times their bounds, CERTAINLY FALSE below minus that, else uncertain.
  visible    trace_cases' brute force over all triangles for the ray (pos, d), with K e as the direction's bound:
             certainly occluded: a robustly hit triangle with t + bound_t < t_max; possibly occluded: any candidate with t - bound_t < t_max, or a
             candidate-list overflow; else certainly visible.
  interval   certainly visible, signs certain: [g - eg, g + eg];  certainly occluded or a sign certainly false: [0, 0];  anything else: [0, g + eg].
A texel's F must lie in (w / S) times the sum of its samples' intervals, widened by K U (S + 4) sum |terms| for the accumulation's roundings, w's own and
the two final operations.  stats[0] (rays traced) and stats[1] (visible ones) must lie between the certain and the possible counts over the LIST (a
duplicate counts again).  A record the rule refuses gives exactly 0 and no ray.
CAPS (from the reference alone): no candidate list overflows; at most 1 % of a case's traced samples have uncertain visibility; at most 2 % of its
texels contain such a sample.
"""
import math

import numpy as np

import atlas_bake_cases as AB
import trace_cases as TC
from texture_cases import K, TINY, U

F32, F64 = np.float32, np.float64
CAP_UNCERTAIN_SAMPLES = 0.01
CAP_UNCERTAIN_TEXELS = 0.02
TAU32, FOURPI32 = F32(6.28318548202514648), F32(12.5663709640502930)
SWC_LO, SWC_HI = F32(1e-6), F32(1.0 - 1e-6)
T_MAX_DEFAULT = 0.999
SENTINEL = 7.0


# ---- records: the layout restated (the records the rule refuses cannot be made with texir_code_amd.irtlight, which refuses them too) ---------------------------

def quad(o, a, b):
    r = np.zeros(16, F32)
    r[0], r[1:4], r[4:7], r[7:10] = 0.0, o, a, b
    return r


def sphere(c, r_):
    r = np.zeros(16, F32)
    r[0], r[1:4], r[4] = 1.0, c, r_
    return r


def record_kind(rec):
    """the rule's own reading of a record: 'quad' | 'sphere' | None (F = 0, no ray)"""
    rec = np.asarray(rec, F32)
    with np.errstate(all="ignore"):
        if rec[0] == 0.0:
            a, b = rec[4:7], rec[7:10]
            m = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
            return "quad" if np.isfinite(rec[1:10]).all() and np.isfinite(m).all() and m.any() else None
        if rec[0] == 1.0:
            w = (FOURPI32 * rec[4]) * rec[4]
            return "sphere" if np.isfinite(rec[1:5]).all() and rec[4] > 0 and np.isfinite(w) else None
    return None


# ---- the sample point in float32 ------------------------------------------------------------------------------------------------------------------------------

def ham0_f32(i, S):
    i = np.asarray(i, np.uint32)
    if S & (S - 1) == 0:
        return i.astype(F32) * (F32(1) / F32(S))
    return (i.astype(F64) / F64(S)).astype(F32)


def ham1_f32(i):
    v = np.asarray(i, np.uint32).copy()
    r = np.zeros_like(v)
    for _ in range(32):
        r = (r << np.uint32(1)) | (v & np.uint32(1))
        v = v >> np.uint32(1)
    return r.astype(F32) * F32(2.0 ** -32)


def shift_wrap_clamp_f32(s, shift):
    s = (s + shift).astype(F32)
    s = np.where(s > F32(1), s - F32(1), s).astype(F32)
    s = np.where(s < F32(0), s + F32(1), s).astype(F32)
    return np.minimum(np.maximum(s, SWC_LO), SWC_HI).astype(F32)


def sample_points(shift, S, mut=None):
    """shift [n,2] f32 -> s0, s1 [n,S] f32"""
    shift = np.asarray(shift, F32).reshape(-1, 2)
    if mut == "shift_ignored":
        shift = np.zeros_like(shift)
    i = np.arange(S, dtype=np.uint32)
    s0 = shift_wrap_clamp_f32(ham0_f32(i, S)[None, :], shift[:, 0:1])
    s1 = shift_wrap_clamp_f32(ham1_f32(i)[None, :], shift[:, 1:2])
    return (s1, s0) if mut == "swap_s0_s1" else (s0, s1)


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------------------------------

def geometry64(x, n, s0, s1, rec):
    """x, n [P,3]; s0, s1 [P,S] (float32 values); rec: a record the rule accepts -> dict of [P,S] (d, e: [P,S,3]) float64 arrays, bounds WITHOUT K"""
    kind = record_kind(rec)
    rec = np.asarray(rec, F32).astype(F64)
    x, n = np.asarray(x, F64)[:, None, :], np.asarray(n, F64)[:, None, :]
    s0, s1 = np.asarray(s0, F64)[..., None], np.asarray(s1, F64)[..., None]
    with np.errstate(all="ignore"):
        if kind == "quad":
            o, a, b = rec[1:4], rec[4:7], rec[7:10]
            p1, p2 = s0 * a, s1 * b
            y = (o + p1) + p2
            d = y - x
            e = U * (3 * (np.abs(o) + np.abs(p1) + np.abs(p2)) + np.abs(d))
            m = np.broadcast_to(np.cross(a, b), d.shape)
            f = np.broadcast_to(2 * U * np.array([abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]), abs(a[0] * b[1]) + abs(a[1] * b[0])]), d.shape)
            w = 1.0
        elif kind == "sphere":
            c, r = rec[1:4], rec[4]
            z = 1 - 2 * s0[..., 0]
            dz = U * np.abs(z)
            A = 1 - z * z
            dA = 2 * np.abs(z) * dz + U * z * z + U * np.abs(A)
            q = np.sqrt(np.maximum(A, 0))
            lin = dA / (2 * np.sqrt(np.maximum(A - dA, 0)))
            dq = np.minimum(np.where(np.isfinite(lin), lin, np.inf), np.sqrt(dA)) + U * q
            phi = 2 * math.pi * s1[..., 0]
            dphi = 1.5 * U * phi
            co, si = np.cos(phi), np.sin(phi)
            dco, dsi = dphi + 8 * U * np.abs(co), dphi + 8 * U * np.abs(si)
            m = np.stack([q * co, q * si, z], -1)
            f = np.stack([np.abs(co) * dq + q * dco + U * np.abs(m[..., 0]), np.abs(si) * dq + q * dsi + U * np.abs(m[..., 1]), dz], -1)
            y = c + r * m
            d = y - x
            e = r * f + U * (np.abs(r * m) + np.abs(y) + np.abs(d))
            w = 4 * math.pi * r * r
        else:
            raise ValueError("geometry64 takes records the rule accepts")
        dd = (d * d).sum(-1)
        ddd = 3 * U * dd + 2 * (np.abs(d) * e).sum(-1)
        nd, md = (n * d).sum(-1), -(m * d).sum(-1)
        dnd = 3 * U * (np.abs(n) * np.abs(d)).sum(-1) + (np.abs(n) * e).sum(-1) + 3 * TINY
        dmd = 3 * U * (np.abs(m) * np.abs(d)).sum(-1) + (np.abs(m) * e).sum(-1) + (np.abs(d) * f).sum(-1) + 3 * TINY
        g = np.maximum(nd, 0) * np.maximum(md, 0) / (dd * dd)
        eg = g * (3 * U + 2 * ddd / dd) + (dnd * np.abs(md) + np.abs(nd) * dmd) / (dd * dd) + 3 * TINY
        zero_n = ~n.any(-1)                                                         # a seam texel: nd = +-0 exactly in float32 too, nd > 0 is certainly false
        yes = (dd > 0) & (nd > K * dnd) & (md > K * dmd) & ~zero_n
        no = ~(dd > 0) | (nd < -K * dnd) | (md < -K * dmd) | zero_n
    return dict(d=d, e=e, g=g, eg=K * eg, yes=yes, no=no, w=w)


class Case:
    """pos, nrm [Nt,3], shift [Nt,2] f32; ids: int32 list | None (= all Nt); lights [K,16] f32; S; t_max"""

    def __init__(self, name, geo, pos, nrm, shift, ids, lights, S, t_max=T_MAX_DEFAULT):
        self.name, self.geo = name, geo
        self.pos, self.nrm = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.Nt = self.pos.shape[0]
        self.shift = np.ascontiguousarray(shift, F32).reshape(self.Nt, 2)
        self.ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
        self.lights = np.ascontiguousarray(lights, F32).reshape(-1, 16)
        self.K, self.S, self.t_max = self.lights.shape[0], int(S), float(F32(t_max))
        self._ref = None

    def listed(self):
        return np.arange(self.Nt, dtype=np.int64) if self.ids is None else self.ids.astype(np.int64)

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref


class Ref:
    def __init__(self, case):
        self.case = c = case
        L = np.unique(c.listed())
        self.tex = L
        n, S = len(L), c.S
        s0, s1 = sample_points(c.shift[L], S)
        self.lo, self.hi, self.mid = np.zeros((c.K, n, S)), np.zeros((c.K, n, S)), np.zeros((c.K, n, S))
        self.w = np.zeros(c.K)
        self.traced_yes, self.traced_maybe = np.zeros((c.K, n, S), bool), np.zeros((c.K, n, S), bool)
        self.vis_yes, self.vis_maybe = np.zeros((c.K, n, S), bool), np.zeros((c.K, n, S), bool)
        self.uncertain_vis = np.zeros((c.K, n, S), bool)
        self.n_overflow = 0
        for k in range(c.K):
            if record_kind(c.lights[k]) is None:
                continue
            G = geometry64(c.pos[L], c.nrm[L], s0, s1, c.lights[k])
            self.w[k] = G["w"]
            ii, ss = np.nonzero(~G["no"])
            self.traced_yes[k], self.traced_maybe[k] = G["yes"], ~G["no"]
            if not len(ii):
                continue
            dr = G["d"][ii, ss]
            rr = TC.RayRef(c.geo, c.pos.astype(F64)[L][ii], dr, K * G["e"][ii, ss] + TINY)
            with np.errstate(invalid="ignore"):
                occ = (rr.has & (rr.c["robust"] > 0) & (rr.t + rr.bt < c.t_max)).any(1)
                maybe = (rr.has & (rr.t - rr.bt < c.t_max)).any(1) | rr.overflow
            self.n_overflow += int(rr.overflow.sum())
            vis = ~maybe
            sure = G["yes"][ii, ss]
            g, eg = G["g"][ii, ss], G["eg"][ii, ss]
            self.lo[k, ii, ss] = np.where(vis & sure, np.maximum(g - eg, 0.0), 0.0)
            self.hi[k, ii, ss] = np.where(occ, 0.0, g + eg)
            self.mid[k, ii, ss] = np.where(occ, 0.0, g)
            self.vis_yes[k, ii, ss], self.vis_maybe[k, ii, ss] = vis & sure, ~occ
            self.uncertain_vis[k, ii, ss] = ~vis & ~occ
        acc = K * (U * (S + 4) * self.hi.sum(2) + (S + 4) * TINY)
        scale = (self.w / S)[:, None]
        self.F_lo, self.F_hi, self.F_mid = scale * (self.lo.sum(2) - acc), scale * (self.hi.sum(2) + acc), scale * self.mid.sum(2)
        self.row_of = {int(t_): i for i, t_ in enumerate(L)}

    def caps(self):
        """(overflowing rays, share of the traced samples whose visibility is uncertain, share of the texels that contain one)"""
        traced = int(self.traced_maybe.sum())
        return (self.n_overflow, float(self.uncertain_vis.sum()) / max(traced, 1), float(self.uncertain_vis.any(2).any(0).mean()) if len(self.tex) else 0.0)

    def counts(self):
        """over the LIST (duplicates count again): (traced lo, traced hi, visible lo, visible hi)"""
        c = self.case
        rows = np.array([self.row_of[int(t)] for t in c.listed() if 0 <= t < c.Nt], np.int64)
        f = lambda a: int(a[:, rows].sum())
        return f(self.traced_yes), f(self.traced_maybe), f(self.vis_yes), f(self.vis_maybe)

    def summary(self):
        over, us, ut = self.caps()
        tr = int(self.traced_maybe.sum())
        occ = int((self.traced_maybe & ~self.vis_maybe).sum())
        return {"texels": len(self.tex), "traced": tr, "occluded_share": occ / max(tr, 1), "uncertain": int(self.uncertain_vis.sum()), "overflow": over,
                "lit_share": [float((self.F_mid[k] > 0).mean()) for k in range(self.case.K)]}


def check(case, F, stats=None, sentinel=None):
    """F [K,Nt]: every listed texel inside its interval (a refused record: exactly 0), unlisted texels keep `sentinel`, stats inside its counts
    -> (list of failure strings (empty: accepted), worst share of an interval: |F - centre| / half width over the texels with a non-empty interval)"""
    ref = case.ref()
    F = np.asarray(F, F64).reshape(case.K, case.Nt)
    fails, worst = [], 0.0
    got = F[:, ref.tex]
    if not np.isfinite(got).all():
        fails.append("non-finite values")
    bad = ~((got >= ref.F_lo) & (got <= ref.F_hi))
    for k, i in np.argwhere(bad)[:8]:
        fails.append("light %d texel %d: %.9g outside [%.9g, %.9g]" % (k, ref.tex[i], got[k, i], ref.F_lo[k, i], ref.F_hi[k, i]))
    if bad.sum() > 8:
        fails.append("... %d values outside in all" % int(bad.sum()))
    half = (ref.F_hi - ref.F_lo) / 2
    with np.errstate(all="ignore"):
        share = np.where(half > 0, np.abs(got - (ref.F_hi + ref.F_lo) / 2) / half, 0.0)
    if share.size and np.isfinite(share).all():
        worst = float(share.max())
    if sentinel is not None:
        un = np.setdiff1d(np.arange(case.Nt), ref.tex)
        if un.size and not (F[:, un] == sentinel).all():
            fails.append("unlisted texels were written")
    if stats is not None:
        t_lo, t_hi, v_lo, v_hi = ref.counts()
        s = [int(v) for v in np.asarray(stats).reshape(-1)[:2]]
        if not (t_lo <= s[0] <= t_hi):
            fails.append("stats[0] = %d outside [%d, %d]" % (s[0], t_lo, t_hi))
        if not (v_lo <= s[1] <= v_hi):
            fails.append("stats[1] = %d outside [%d, %d]" % (s[1], v_lo, v_hi))
    return fails, worst


def all_certain(case):
    """[K, n listed-unique] bool: every sample of the texel has certain signs and certain visibility (the texels the restatement binds on)"""
    r = case.ref()
    return ~(r.uncertain_vis | (r.traced_maybe & ~r.traced_yes)).any(2)


def rounding_bound(case):
    """[K, n]: the header's bound on F alone (no visibility or sign alternatives): (w / S) (K (S + 4) u sum g + sum eg); two float32 evaluations of the
    rule on certain texels differ by at most twice this"""
    r = case.ref()
    return r.F_hi - r.F_mid


# ---- float32 restatement of the kernel's arithmetic (CPU), op by op, with the mutants the checker must reject ----------------------------------------------------

MUTANTS = ("no_visibility", "two_sided", "no_texel_cosine", "r2_falloff", "half_sphere_area", "shift_ignored", "t_max_1", "swap_s0_s1")


def lights_f32(case, mut=None, sentinel=SENTINEL, trace=None):
    """-> (F [K,Nt] f32, stats [2]); unlisted texels hold the sentinel.  trace(org [R,3], dir [R,3]) -> (t [R], pid [R]); default: trace_cases.trace_f32"""
    c = case
    F = np.full((c.K, c.Nt), sentinel, F32)
    stats = np.zeros(2, np.int64)
    lst = c.listed()
    lst = lst[(lst >= 0) & (lst < c.Nt)]
    L, inv = np.unique(lst, return_inverse=True)
    mult = np.bincount(inv, minlength=len(L))                                      # a duplicate is traced again
    x, nr = c.pos[L], c.nrm[L]
    n, S = len(L), c.S
    s0, s1 = sample_points(c.shift[L], S, mut)
    t_max = F32(1.0) if mut == "t_max_1" else F32(c.t_max)
    one = F32(1)
    for k in range(c.K):
        rec = c.lights[k]
        kind = record_kind(rec)
        if kind is None:
            F[k, L] = 0
            continue
        o, a, b = rec[1:4], rec[4:7], rec[7:10]
        with np.errstate(all="ignore"):
            if kind == "quad":
                y = [(o[i] + s0 * a[i]) + s1 * b[i] for i in range(3)]
                m = [np.full((n, S), v, F32) for v in (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])]
                w = one
            else:
                r = a[0]
                z = one - F32(2) * s0
                q = np.sqrt(np.maximum(F32(0), one - z * z))
                phi = TAU32 * s1
                m = [q * np.cos(phi).astype(F32), q * np.sin(phi).astype(F32), z]
                y = [o[i] + r * m[i] for i in range(3)]
                w = (FOURPI32 * r) * r
                if mut == "half_sphere_area":
                    w = (F32(0.5) * FOURPI32 * r) * r
            d = [(y[i] - x[:, i:i + 1]).astype(F32) for i in range(3)]
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nd = (nr[:, 0:1] * d[0] + nr[:, 1:2] * d[1]) + nr[:, 2:3] * d[2]
            md = -((m[0] * d[0] + m[1] * d[1]) + m[2] * d[2])
            if mut == "two_sided":
                md = np.abs(md)
            if mut == "no_texel_cosine":
                nd = np.sqrt(dd)
            den = dd if mut == "r2_falloff" else dd * dd
            g = ((nd * md) / den).astype(F32)
            g = np.where((nd > 0) & (md > 0) & (dd > 0) & np.isfinite(g), g, F32(0)).astype(F32)
        ii, ss = np.nonzero(g > 0)
        vis = np.zeros((n, S), bool)
        if len(ii):
            if mut == "no_visibility":
                v = np.ones(len(ii), bool)
            else:
                dirs = np.stack([d[0][ii, ss], d[1][ii, ss], d[2][ii, ss]], 1)
                t, pid = (trace or (lambda o_, d_: TC.trace_f32(c.geo, o_, d_)[:2]))(x[ii], dirs)
                v = ~((pid >= 0) & (t < t_max))
            vis[ii, ss] = v
        stats[0] += int(((g > 0) * mult[:, None]).sum())
        stats[1] += int((vis * mult[:, None]).sum())
        acc = np.zeros(n, F32)
        for s in range(S):
            acc = np.where(vis[:, s], acc + g[:, s], acc).astype(F32)
        F[k, L] = (acc * w) / F32(S)
    return F, stats


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------------------

_CACHE = {}


def room_inputs():
    """atlas_bake_cases.room(64) with seeded shifts: (geo, pos, nrm, shift [Nt,2], valid ids in Morton order, lo, hi)"""
    if "room" not in _CACHE:
        geo, pos, nrm, v = AB.room(64)
        shift = np.random.default_rng(41).random((pos.shape[0], 2), dtype=F32)
        lo, hi = geo.verts.min(0).astype(F64), geo.verts.max(0).astype(F64)
        _CACHE["room"] = (geo, pos, nrm, shift, AB.morton(v, 64), lo, hi)
    return _CACHE["room"]


def room_quad_record():
    """the cases' valid lights are made with the shipped helpers (irtlight.quad / irtlight.sphere): the records under test are the ones a user gets"""
    from texir_code_amd import irtlight
    _, _, _, _, _, lo, hi = room_inputs()
    ext, c = hi - lo, (hi + lo) / 2
    a, b = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    centre = np.array([c[0], hi[1] - 0.15 * ext[1], c[2]])
    return irtlight.quad(centre - a / 2 - b / 2, a, b)                             # a x b = (0, -|a||b|, 0): it shines down


def room_sphere_record():
    from texir_code_amd import irtlight
    _, _, _, _, _, lo, hi = room_inputs()
    ext, c = hi - lo, (hi + lo) / 2
    return irtlight.sphere([c[0], lo[1] + 0.6 * ext[1], c[2]], 0.05 * ext.min())


def room_eight_records():
    _, _, _, _, _, lo, hi = room_inputs()
    ext, c = hi - lo, (hi + lo) / 2
    a, b = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    nan_rec = room_quad_record().copy()
    nan_rec[1] = np.nan
    other = room_sphere_record().copy()
    other[0] = 2.0
    return np.stack([
        room_quad_record(),
        quad([c[0] - 0.5, hi[1], c[2] - 0.5], b / np.linalg.norm(b), a / np.linalg.norm(a)),            # in the ceiling plane, b x a: it faces the ceiling -- all zero
        room_sphere_record(),
        quad([c[0], c[1], c[2]], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]),                                      # zero area
        sphere([c[0], c[1], c[2]], 0.0),                                                                 # r = 0
        nan_rec,
        other,                                                                                           # unknown kind
        quad([lo[0] + 0.25 * ext[0], lo[1] + 0.5 * ext[1], lo[2] + 0.25 * ext[2]], [0.5, 0.25, 0.125], [-0.125, 0.25, 0.5]),      # tilted: every component of m
    ])


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng([43, len(name)])
    if name in ("room_quad", "room_sphere", "room_eight"):
        geo, pos, nrm, shift, ids, _, _ = room_inputs()
        if name == "room_quad":
            c = Case(name, geo, pos, nrm, shift, ids, room_quad_record()[None], 16)
        elif name == "room_sphere":
            c = Case(name, geo, pos, nrm, shift, ids, room_sphere_record()[None], 16)
        else:
            c = Case(name, geo, pos, nrm, shift, ids[1::6], room_eight_records(), 16)
    elif name.startswith("list"):
        n, S, order = {"list1": (1, 64, "morton"), "list63": (63, 17, "shuffled"), "list64": (64, 1, "morton"), "list65": (65, 2, "shuffled"),
                       "list200": (200, 64, "morton")}[name]
        geo, pos, nrm, shift, v, _, _ = room_inputs()
        ids = v[7::max(1, len(v) // n - 1)][:n]
        if n == 1:
            ids = v[len(v) // 2:][:1]
        assert len(ids) == n
        if order == "shuffled":
            ids = rng.permutation(ids)
        c = Case(name, geo, pos, nrm, shift, ids, np.stack([room_quad_record(), room_sphere_record()]), S)
    elif name == "null200":
        # texel_ids NULL: all Nt = 200 texels of a compacted G-buffer, seams (zero normals) among them
        geo, pos, nrm, shift, v, _, _ = room_inputs()
        v = np.sort(v)
        pick = np.concatenate([v[5::len(v) // 190][:190], np.setdiff1d(np.arange(64 * 64), v)[:10]])
        c = Case(name, geo, pos[pick], nrm[pick], shift[pick], None, np.stack([room_sphere_record(), room_quad_record()]), 16)
    elif name == "closed_box":
        # the bake's case: texels INSIDE the closed cube, the lights outside: nobody sees them, every F is exactly 0 and nothing is visible
        b = AB.case("closed_box")
        shift = rng.random((b.Nt, 2), dtype=F32)
        lights = np.stack([quad([2.5, -0.5, -0.5], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]),                    # a x b = (-1, 0, 0): it faces the cube
                           sphere([0.25, 3.0, -0.5], 0.5), sphere([-0.5, 0.25, -2.75], 0.25)])
        c = Case(name, b.geo, b.pos, b.nrm, shift, None, lights, 16)
    elif name == "on_surface":
        # a quad lying IN the floor plane y = -1 of the cube, facing up, dyadic coordinates: its own floor is hit at t = 1 and must not shadow it
        geo = TC.box_grid_geo(8)
        e = 2.0 ** -6
        pts, nrs = [], []
        for i in range(24):                                                        # the four walls and the ceiling, offset inwards by 2^-6
            u_, v_ = -0.8125 + 0.0625 * (i % 6) * 5, -0.6875 + 0.375 * (i // 6)
            pts += [(-1 + e, v_, u_), (1 - e, v_, u_), (u_, v_, -1 + e), (u_, v_, 1 - e), (u_, 1 - e, v_)]
            nrs += [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0)]
        for i in range(8):                                                         # floor texels: the light lies below their offset positions
            pts.append((-0.75 + 0.1875 * i, -1 + e, 0.3125))
            nrs.append((0, 1, 0))
        pos, nrm = np.array(pts, F32), np.array(nrs, F32)
        shift = rng.random((len(pos), 2), dtype=F32)
        lights = quad([-0.3125, -1.0, -0.4375], [0.0, 0.0, 0.75], [0.5, 0.0, 0.0])[None]                 # a x b = (0, 0.375, 0): up
        c = Case(name, geo, pos, nrm, shift, None, lights, 16)
    else:
        raise KeyError(name)
    _CACHE[name] = c
    return c


ALL = ("room_quad", "room_sphere", "room_eight", "closed_box", "on_surface", "list1", "list63", "list64", "list65", "list200", "null200")
# where each mutant must be rejected
MUTANT_CASES = {"no_visibility": "list63", "two_sided": "list63", "no_texel_cosine": "list63", "r2_falloff": "list63", "half_sphere_area": "list63",
                "shift_ignored": "list63", "t_max_1": "on_surface", "swap_s0_s1": "list63"}


# ---- the closed forms of the header's geometry (no occluder) -------------------------------------------------------------------------------------------------------

def unoccluded_F(x, n, shift, rec, S):
    """F of one point without any geometry in the way, from the float64 reference alone"""
    s0, s1 = sample_points(np.asarray(shift, F32).reshape(1, 2), S)
    G = geometry64(np.asarray(x, F32).reshape(1, 3), np.asarray(n, F32).reshape(1, 3), s0, s1, rec)
    return float(G["w"] / S * G["g"].sum())


def corner_form_factor(a, b, h):
    """pi F_d1-2 of a differential element under the corner of a parallel a x b rectangle at height h"""
    A, B = a / h, b / h
    return 0.5 * (A / math.sqrt(1 + A * A) * math.atan(B / math.sqrt(1 + A * A)) + B / math.sqrt(1 + B * B) * math.atan(A / math.sqrt(1 + B * B)))
