"""Float64 classification of occlusion queries (include/texir_hip.h, texir_trace_occluded: is some triangle accepted with t_near < t < t_far?), the checks of an
answer against it, the float32 restatement with its mutants, and the cases.  Shared by test_occlusion_ref_cpu.py (no GPU) and test_gpu_occlusion.py; no tests
here.  Built on trace_cases: Geo, candidates_numpy / RayRef, bound_t, and its candidate and robustly-hit rules (K = 4, U, TINY are texture_cases').  Nothing in
this module comes from a kernel.

PER RAY AND SEGMENT (t_near, t_far), with every triangle's exact t, its bound_t (K included) and trace_cases' two rules (a CANDIDATE has min_i w_i > -m and
t + bound_t > 0; it is ROBUSTLY HIT when min_i w_i >= m and t - bound_t > 0):
    certainly occluded   some robustly hit triangle has t - bound_t > t_near and t + bound_t < t_far;
    certainly visible    no candidate has t + bound_t > t_near and t - bound_t < t_far;
    uncertain            anything else: both answers pass.
The lists are the FULL lists over all triangles (candidates_numpy in chunks), not RayRef's, which stop behind the closest robust hit: a segment that starts
at t_near > 0 looks behind it.  At t_near = 0 RayRef's lists give the same classes (classify_rayref; the CPU test asserts the agreement): if any robust triangle
ends before t_far, so does the one that ends first, and that one is on the list; a candidate cut from the list starts behind that end.

THE SECOND CHECK is an identity, not a bound: at t_near = 0 the answer must equal `hit & (t_hit < t_far)` of the closest-hit query of the same arithmetic on
EVERY ray (equals_closest).  This is what rejects `t <= t_far` on an exact tie, where the classes above say "uncertain".

SEGMENTS of a case: t_far in (inf, 1, a value near the median closest robust t), t_near in (0, a value near the lower quartile).  "Near": the quantile
times 1 + 2^-5 (t_far) or 1 - 2^-5 (t_near), rounded to float32, so that the bound does not sit on the quantile ray's own hit.
CAP (from the reference alone, asserted by the CPU test): at most 2 % of a case's rays are uncertain in any of its segments (trace_cases.CAP_MULTI).  The
cap is a condition on the case, so the cases that miss it with the segments above take other segments, never another cap:
    patho_fan, patho_single, patho_stack   the rays END on the flat mesh (target points in its plane: t = 1): 1.25 for 1 (FAR_ONE);
    grid_on_face                           two thirds of the rays START on a face (a candidate at t = 0 +- bound_t): 2^-12 for t_near = 0 (NEAR_ZERO);
    grid_vertices_edges, grid_axis_parallel  every ray is aimed at a shared vertex or edge, runs inside a face or meets a grid line head-on: NO triangle is
                                           robustly hit, so every segment that holds the surface is uncertain for every ray.  Their segments for THIS check
                                           end before the surface or start behind it (SEGMENTS_FIXED: certainly visible); that such a ray does not leak
                                           through the shared vertex is bound by the identity below on the standard segments (equal_segments), ray by ray.
"""
import numpy as np

import trace_cases as TC
from texture_cases import K

F32, F64 = np.float32, np.float64
CAP_UNCERTAIN = TC.CAP_MULTI
INF = float("inf")
# t_far of the "one" segment where 1 is the rays' own end point on the geometry
FAR_ONE = {"patho_fan": 1.25, "patho_single": 1.25, "patho_stack": 1.25}
NEAR_ZERO = {"grid_on_face": 2.0 ** -12}
# (from (0.125, -0.25, 0.0625), directions of twice the vector to the target: every hit at t = 0.5;  axis-parallel: hits at t = 2/3, 1.5 and 2.5, grazing up to 2/3)
SEGMENTS_FIXED = {"grid_vertices_edges": (("before", 0.0, 0.4375), ("behind_inf", 0.5625, INF), ("behind_one", 0.5625, 1.0)),
                  "grid_axis_parallel": (("between", 0.75, 1.25), ("between2", 1.75, 2.25), ("behind_inf", 2.75, INF))}
PAIRS_PER_CHUNK = 60000


# ---- the full lists ------------------------------------------------------------------------------------------------------------------------------------------

class Lists:
    """every triangle that passes trace_cases' candidate rule without the cut behind the closest robust hit, per ray: ragged arrays ray [M], t [M], bt [M]
    (K included), robust [M]"""

    def __init__(self, geo, org, dir):
        org, dir = np.asarray(org, F64).reshape(-1, 3), np.asarray(dir, F64).reshape(-1, 3)
        self.R = R = org.shape[0]
        step = max(1, PAIRS_PER_CHUNK // max(geo.T, 1))
        ray, t, bt, rob = [], [], [], []
        for s in range(0, R, step):
            c = TC.candidates_numpy(geo, org[s:s + step], dir[s:s + step])
            d = dir[s:s + step]
            live = np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0)                  # a zero or non-finite direction has no candidate
            with np.errstate(all="ignore"):
                pre = live[:, None] & np.isfinite(c["t"]) & (c["minb"] > -c["m"]) & (c["t"] + K * c["bt"] > 0)
                # the pin: trace_cases' own lists are this one cut behind the closest robust hit
                assert not (c["robust"] & ~pre).any() and np.array_equal(c["cand"], pre & (c["t"] - K * c["bt"] <= c["tlim"][:, None]))
            i, j = np.nonzero(pre)
            ray.append(i + s)
            t.append(c["t"][i, j])
            bt.append(K * c["bt"][i, j])
            rob.append(c["robust"][i, j])
        self.ray, self.t, self.bt, self.robust = (np.concatenate(a) if a else np.zeros(0, d) for a, d in ((ray, np.int64), (t, F64), (bt, F64), (rob, bool)))

    def classify(self, t_near, t_far):
        """-> (certainly occluded [R], certainly visible [R])"""
        t_near, t_far = float(t_near), float(t_far)
        with np.errstate(invalid="ignore"):
            yes = self.robust & (self.t - self.bt > t_near) & (self.t + self.bt < t_far)
            maybe = (self.t + self.bt > t_near) & (self.t - self.bt < t_far)
        occ, may = np.zeros(self.R, bool), np.zeros(self.R, bool)
        occ[self.ray[yes]] = True
        may[self.ray[maybe]] = True
        return occ, ~may

    def closest_robust(self):
        """exact t of the closest robustly hit triangle per ray (inf: none)"""
        out = np.full(self.R, np.inf)
        np.minimum.at(out, self.ray[self.robust], self.t[self.robust])
        return out


def classify_rayref(rr, t_far):
    """the same classes at t_near = 0 from a trace_cases.RayRef (its lists stop behind the closest robust hit; a direction bound is part of its bound_t)
    -> (certainly occluded, certainly visible); a ray whose list overflowed is uncertain"""
    with np.errstate(invalid="ignore"):
        occ = (rr.has & (rr.c["robust"] > 0) & (rr.t - rr.bt > 0) & (rr.t + rr.bt < t_far)).any(1)
        maybe = (rr.has & (rr.t + rr.bt > 0) & (rr.t - rr.bt < t_far)).any(1) | rr.overflow
    return occ, ~maybe


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------------------------

def check_certain(occ, vis, got, what=""):
    """got [R] bool: every certain ray has its answer -> the number of uncertain rays; raises AssertionError naming the rays that fail"""
    got = np.asarray(got).astype(bool).reshape(-1)
    assert got.shape == occ.shape, (got.shape, occ.shape)
    bad = np.nonzero((occ & ~got) | (vis & got))[0]
    if bad.size:
        raise AssertionError("%s: %d of %d rays against the reference: %s" % (what, bad.size, len(got), ", ".join(
            "ray %d %s, certainly %s" % (i, "occluded" if got[i] else "visible", "occluded" if occ[i] else "visible") for i in bad[:8])))
    return int((~occ & ~vis).sum())


def equals_closest(got, t_hit, pid, t_far, what=""):
    """the identity at t_near = 0: got == hit & (t_hit < t_far) on every ray (t_hit, pid: the closest-hit query's float32 results)"""
    got = np.asarray(got).astype(bool).reshape(-1)
    with np.errstate(invalid="ignore"):
        want = (np.asarray(pid).reshape(-1) >= 0) & (np.asarray(t_hit, F32).reshape(-1) < F32(t_far))
    bad = np.nonzero(got != want)[0]
    if bad.size:
        raise AssertionError("%s: %d of %d rays differ from the closest-hit answer (t_far %r): rays %s, t_hit %s" % (what, bad.size, len(got), t_far, bad[:8].tolist(),
                                                                                                                  np.asarray(t_hit).reshape(-1)[bad[:8]].tolist()))


# ---- float32 restatement (CPU): the leaf test of trace_cases.trace_f32, every accepted triangle instead of the closest --------------------------------------

MUTANTS = ("far_ignored", "near_ignored", "t_le_0", "t_le_far", "first_of_leaf")
LEAF = 2                  # the mutant's "leaf": LEAF consecutive triangles, of which it tests the first only


def leaf_f32(geo, org, dir, chunk=96):
    """trace_f32's arithmetic, operation by operation (the documented watertight test) -> (inside [R,T] bool: the accept test without its conditions on t,
    t [R,T] float32).  The CPU test pins this copy to trace_f32: the smallest accepted t > 0 and its triangle are trace_f32's, bit for bit."""
    org, dir = np.ascontiguousarray(org, F32).reshape(-1, 3), np.ascontiguousarray(dir, F32).reshape(-1, 3)
    R = org.shape[0]
    V = geo.verts[geo.tris]
    inside, tt = np.zeros((R, geo.T), bool), np.zeros((R, geo.T), F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for s in range(0, R, chunk):
            o, d = org[s:s + chunk], dir[s:s + chunk]
            r = o.shape[0]
            rr = np.arange(r)
            a = np.abs(d)
            kz = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
            Sz = one / d[rr, kz]
            Sx, Sy = d[rr, (kz + 1) % 3] * Sz, d[rr, (kz + 2) % 3] * Sz
            q = V[None] - o[:, None, None, :]
            pick = lambda ax: q[rr[:, None, None], np.arange(geo.T)[None, :, None], np.arange(3)[None, None, :], ax[:, None, None]]
            qx, qy, qz = pick((kz + 1) % 3), pick((kz + 2) % 3), pick(kz)
            e_ = lambda x: x[:, None, None]
            fma = lambda x, y, z: (x.astype(F64) * y.astype(F64) + z.astype(F64)).astype(F32)
            X, Y, Z = fma(-e_(Sx), qz, qx), fma(-e_(Sy), qz, qy), e_(Sz) * qz

            def edge(bx, by, cx, cy):
                p, qq = cx * by, cy * bx
                e = p - qq
                z = e == 0
                if z.any():
                    e = np.where(z, fma(cx, by, -p) - fma(cy, bx, -qq), e)
                return e
            Ue = edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2])
            Ve = edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0])
            We = edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1])
            mn, mx = np.minimum(np.minimum(Ue, Ve), We), np.maximum(np.maximum(Ue, Ve), We)
            det = (Ue + Ve) + We
            inv = one / det
            tt[s:s + r] = ((Ue * Z[..., 0] + Ve * Z[..., 1]) + We * Z[..., 2]) * inv
            inside[s:s + r] = ~((mn < 0) & (mx > 0)) & (det != 0)
    return inside, tt


def occluded_f32(geo, org, dir, t_near, t_far, mut=None, leaf=None):
    """the rule in float32: some triangle inside with t_near < t < t_far.  leaf: a cached leaf_f32 result.  mut: one of MUTANTS"""
    inside, t = leaf_f32(geo, org, dir) if leaf is None else leaf
    tn, tf = F32(t_near), F32(t_far)
    if mut == "far_ignored":
        tf = F32(np.inf)
    if mut == "near_ignored":
        tn = F32(0)
    with np.errstate(invalid="ignore"):
        ok = inside & (t < tf if mut != "t_le_far" else t <= tf)
        if mut != "t_le_0":
            ok &= t > tn
    if mut == "first_of_leaf":
        ok = ok & (np.arange(geo.T) % LEAF == 0)[None, :]
    return ok.any(1)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------

class OccCase:
    def __init__(self, name, geo, org, dir):
        self.name, self.geo = name, geo
        self.org, self.dir = np.ascontiguousarray(org, F32).reshape(-1, 3), np.ascontiguousarray(dir, F32).reshape(-1, 3)
        self.R = self.org.shape[0]
        self._lists = self._seg = self._leaf = None
        self._cls = {}

    def lists(self):
        if self._lists is None:
            self._lists = Lists(self.geo, self.org, self.dir)
        return self._lists

    def equal_segments(self):
        """the segments of the identity with the closest-hit query: t_near = 0 and the three standard far ends, for every case"""
        return [(tag, tn, tf) for tag, tn, tf in self.segments(fixed=False) if tag.startswith("zero_")]

    def segments(self, fixed=True):
        """[(tag, t_near, t_far)]: 3 far ends x 2 near ends, float32 values (fixed: a case of SEGMENTS_FIXED gives those instead)"""
        if fixed and self.name in SEGMENTS_FIXED:
            return list(SEGMENTS_FIXED[self.name])
        if self._seg is None:
            tc = self.lists().closest_robust()
            tc = tc[np.isfinite(tc)]
            med = float(F32(np.median(tc) * (1 + 2.0 ** -5))) if tc.size else 0.75
            q25 = float(F32(np.quantile(tc, 0.25) * (1 - 2.0 ** -5))) if tc.size else 0.25
            fars = (("inf", INF), ("one", FAR_ONE.get(self.name, 1.0)), ("median", med))
            self._seg = [("%s_%s" % (nn, fn), tn, tf) for nn, tn in (("zero", 0.0), ("q25", q25)) for fn, tf in fars]
        if fixed and self.name in NEAR_ZERO:
            return [(tag, NEAR_ZERO[self.name] if tag.startswith("zero_") else tn, tf) for tag, tn, tf in self._seg]
        return self._seg

    def classify(self, t_near, t_far):
        key = (float(t_near), float(t_far))
        if key not in self._cls:
            self._cls[key] = self.lists().classify(*key)
        return self._cls[key]

    def leaf(self):
        if self._leaf is None:
            self._leaf = leaf_f32(self.geo, self.org, self.dir)
        return self._leaf


_CASES = {}


def tie_case():
    """exact ties: one triangle in the plane z = 0 with dyadic corners, rays along +z of length 2 from z = -1 (t = 0.5 exactly in float32: every operand of
    the leaf test is dyadic and det a power of two) plus the same rays from z = -0.5 (t = 0.25) and rays that miss.  Its segment ends ON the hit: t_far = 0.5"""
    verts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], F32)
    geo = TC.Geo("tie", verts, np.array([[0, 1, 2]], np.int32), np.array([[0, 0], [1, 0], [0, 1]], F32), np.ones((4, 4, 3), F32))
    xy = np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.5], [0.125, 0.125], [3.0, 3.0], [-1.0, 0.5]], F32)
    org = np.concatenate([np.concatenate([xy, np.full((len(xy), 1), z, F32)], 1) for z in (-1.0, -0.5)])
    return OccCase("tie", geo, org, np.tile(np.array([[0, 0, 2]], F32), (len(org), 1)))


def cases():
    """name -> OccCase: trace_cases.ray_cases(small=True) -- the room and the box (random rays, texel hemispheres), house, scan, the four pathological meshes
    (`patho_stack`: the 3000 stacked triangles), the closed grid cube's vertex / edge / face / un-normalised / non-finite rays"""
    if not _CASES:
        for c in TC.ray_cases(small=True):
            _CASES[c.name] = OccCase(c.name, c.geo, c.org, c.dir)
    return _CASES


def case(name):
    if name == "tie":
        if "tie" not in _CASES:
            cases()
            _CASES["tie"] = tie_case()
        return _CASES["tie"]
    return cases()[name]


NAMES = ("room_random", "room_hemisphere", "box_random", "box_hemisphere", "house_random", "scan_random", "patho_stack", "patho_fan", "patho_soup", "patho_single",
         "grid_vertices_edges", "grid_axis_parallel", "grid_on_face", "grid_unnormalised", "grid_zero_nonfinite")
# (mutant, case, segment tag, which check must reject it)
MUTANT_CASES = (("far_ignored", "room_random", "zero_median", "certain"), ("near_ignored", "room_random", "q25_inf", "certain"),
                ("t_le_0", "house_random", "zero_median", "certain"), ("t_le_far", "tie", None, "closest"), ("first_of_leaf", "grid_unnormalised", "zero_inf", "certain"))
TIE_FAR = 0.5


def light_rays(name):
    """the rays light_cases.Ref traces for case `name` (one light), as it builds them: -> (light case, RayRef over the not-certainly-skipped samples, the
    mask [n,S] of those samples)"""
    import light_cases as LC
    from texture_cases import TINY
    c = LC.case(name)
    assert c.K == 1
    L = np.unique(c.listed())
    s0, s1 = LC.sample_points(c.shift[L], c.S)
    G = LC.geometry64(c.pos[L], c.nrm[L], s0, s1, c.lights[0])
    ii, ss = np.nonzero(~G["no"])
    rr = TC.RayRef(c.geo, c.pos.astype(F64)[L][ii], G["d"][ii, ss], K * G["e"][ii, ss] + TINY)
    return c, rr, ~G["no"]
