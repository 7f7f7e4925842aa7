"""Cases of the inserted lights behind inserted mesh objects (include/texir_hip.h texir_irt_lights_mesh, texir_spec_lights_mesh; csrc/irtlightmesh.hip,
csrc/speclightmesh.hip): the float64 references, the float32 restatement with the mutants the check must reject, and the seeded cases.  Shared by
test_irt_lights_mesh_ref_cpu.py (no GPU) and test_gpu_irt_lights_mesh.py; no tests here.  Nothing of light_cases (LC), spec_light_cases (SL),
irt_shadow_mesh_cases (MC), occlusion_cases (OC) or trace_cases (TC) is changed; KF = 4, U = 2^-24 and TINY are texture_cases'; every margin is the header's
ROUNDING BOUND times KF, fixed before any GPU run; nothing is taken from a kernel's output.

THE REFERENCE is LC.Ref (SL.Ref for the specular rule) with the sample's VISIBILITY extended by the instances.  Per instance j with a finite matrix:
  object-space ray   o' in the rule's float32 sequence in numpy (MC.point_f32: a fixed value on any IEEE machine), d' = W d in float64 with the header's bound
                     |W| e + KF 3 u |W| |d|, e the bound of d the light rule gives (KF included)
  brute force        TC.RayRef over the OCCLUDER's triangles along (o', d' +- bound)
  certainly blocked  certainly occluded by the scene (LC's test), or a robustly hit instance triangle with t + bound_t < t_max
  possibly blocked   likewise with t - bound_t < t_max, or a candidate-list overflow
Intervals, the accumulation's widening, check() and counts() are LC's (SL's), used as they are: the classes here have the attributes those functions read.
CAPS (LC's, from the reference alone, asserted per case in the CPU suite): no candidate overflow; at most 1 % of a case's traced samples have uncertain
visibility; at most 2 % of its texels hold such a sample.  The poses below were chosen so that this holds.
"""
import numpy as np

import irt_shadow_mesh_cases as MC
import light_cases as LC
import occlusion_cases as OC
import spec_light_cases as SL
import trace_cases as TC
from texture_cases import K as KF, TINY, U

F32, F64 = np.float32, np.float64
SENTINEL = LC.SENTINEL
CAP_UNCERTAIN_SAMPLES, CAP_UNCERTAIN_TEXELS = LC.CAP_UNCERTAIN_SAMPLES, LC.CAP_UNCERTAIN_TEXELS


# ---- the instances' part of a segment's visibility, float64 ------------------------------------------------------------------------------------------------------

def instance_classes(case, x32, d, bd):
    """x32 [R,3] float32 origins, d [R,3] float64 directions, bd [R,3] their bound (KF included) -> (certainly blocked [R], possibly blocked [R], overflowing
    rays) by the instances alone"""
    R = len(x32)
    occ, maybe, over = np.zeros(R, bool), np.zeros(R, bool), 0
    for j in range(case.J):
        W32 = case.w2o[j]
        if not np.isfinite(W32).all():
            continue                                                               # a matrix with a non-finite entry never blocks
        g = MC.occluder(case.occ[case.inst[j]])
        W = W32.astype(F64).reshape(3, 4)[:, :3]
        o = MC.point_f32(W32, x32).astype(F64)
        d_o = d @ W.T
        bd_o = bd @ np.abs(W).T + KF * (3 * U * (np.abs(d) @ np.abs(W).T) + 3 * TINY)
        rr = TC.RayRef(g, o, d_o, bd_o)
        with np.errstate(invalid="ignore"):
            occ |= (rr.has & (rr.c["robust"] > 0) & (rr.t + rr.bt < case.t_max)).any(1)
            maybe |= (rr.has & (rr.t - rr.bt < case.t_max)).any(1) | rr.overflow
        over += int(rr.overflow.sum())
    return occ, maybe | occ, over


class _Objects:
    """the objects of a case: occ: names of the Q occluders (MC.occluder); inst: occluder index per instance; poses [J,3,4] object-to-world float64, or w2o
    [J,12] float32 world-to-object given directly (the only way to a non-finite matrix)"""

    def set_objects(self, occ, inst, poses=None, w2o=None):
        self.occ, self.inst = list(occ), [int(i) for i in inst]
        self.J = len(self.inst)
        if w2o is not None:
            self.poses, self.w2o = None, np.ascontiguousarray(w2o, F32).reshape(self.J, 12)
        else:
            self.poses = np.asarray(poses, F64).reshape(-1, 3, 4)
            assert len(self.poses) == self.J
            self.w2o = MC.to_world_to_object(self.poses) if self.J else np.zeros((0, 12), F32)


class Case(LC.Case, _Objects):
    """an LC case plus occ, inst, poses"""

    def __init__(self, name, base, occ, inst, poses=None, w2o=None):
        LC.Case.__init__(self, "lm:" + name, base.geo, base.pos, base.nrm, base.shift, base.ids, base.lights, base.S, base.t_max)
        self.base = base
        self.set_objects(occ, inst, poses, w2o)

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref


class Ref(LC.Ref):
    """LC.Ref.__init__ with the instances in the sample's visibility (the same statements; `occ` and `maybe` are extended)"""

    def __init__(self, case):
        self.case = c = case
        L = np.unique(c.listed())
        self.tex = L
        n, S = len(L), c.S
        s0, s1 = LC.sample_points(c.shift[L], S)
        self.lo, self.hi, self.mid = np.zeros((c.K, n, S)), np.zeros((c.K, n, S)), np.zeros((c.K, n, S))
        self.w = np.zeros(c.K)
        self.traced_yes, self.traced_maybe = np.zeros((c.K, n, S), bool), np.zeros((c.K, n, S), bool)
        self.vis_yes, self.vis_maybe = np.zeros((c.K, n, S), bool), np.zeros((c.K, n, S), bool)
        self.uncertain_vis = np.zeros((c.K, n, S), bool)
        self.blocked_by_object = np.zeros((c.K, n, S), bool)                       # certainly blocked by an instance, not certainly by the scene
        self.n_overflow = 0
        for k in range(c.K):
            if LC.record_kind(c.lights[k]) is None:
                continue
            G = LC.geometry64(c.pos[L], c.nrm[L], s0, s1, c.lights[k])
            self.w[k] = G["w"]
            ii, ss = np.nonzero(~G["no"])
            self.traced_yes[k], self.traced_maybe[k] = G["yes"], ~G["no"]
            if not len(ii):
                continue
            dr, bd = G["d"][ii, ss], KF * G["e"][ii, ss] + TINY
            rr = TC.RayRef(c.geo, c.pos.astype(F64)[L][ii], dr, bd)
            with np.errstate(invalid="ignore"):
                occ_s = (rr.has & (rr.c["robust"] > 0) & (rr.t + rr.bt < c.t_max)).any(1)
                maybe = (rr.has & (rr.t - rr.bt < c.t_max)).any(1) | rr.overflow
            self.n_overflow += int(rr.overflow.sum())
            occ_o, maybe_o, over = instance_classes(c, c.pos[L][ii], dr, bd)
            self.n_overflow += over
            occ, maybe = occ_s | occ_o, maybe | maybe_o
            vis = ~maybe
            sure = G["yes"][ii, ss]
            g, eg = G["g"][ii, ss], G["eg"][ii, ss]
            self.lo[k, ii, ss] = np.where(vis & sure, np.maximum(g - eg, 0.0), 0.0)
            self.hi[k, ii, ss] = np.where(occ, 0.0, g + eg)
            self.mid[k, ii, ss] = np.where(occ, 0.0, g)
            self.vis_yes[k, ii, ss], self.vis_maybe[k, ii, ss] = vis & sure, ~occ
            self.uncertain_vis[k, ii, ss] = ~vis & ~occ
            self.blocked_by_object[k, ii, ss] = occ_o & ~occ_s
        acc = KF * (U * (S + 4) * self.hi.sum(2) + (S + 4) * TINY)
        scale = (self.w / S)[:, None]
        self.F_lo, self.F_hi, self.F_mid = scale * (self.lo.sum(2) - acc), scale * (self.hi.sum(2) + acc), scale * self.mid.sum(2)
        self.row_of = {int(t_): i for i, t_ in enumerate(L)}


class SpecCase(SL.Case, _Objects):
    """an SL case plus occ, inst, poses"""

    def __init__(self, name, base, occ, inst, poses=None, w2o=None):
        SL.Case.__init__(self, "sm:" + name, base.geo, base.pos, base.nrm, base.rough, base.shift, base.cam, base.ids, base.lights, base.S, base.t_max, base.ceps)
        self.base = base
        self.set_objects(occ, inst, poses, w2o)

    def ref(self):
        if self._ref is None:
            self._ref = SpecRef(self)
        return self._ref


class SpecRef(SL.Ref):
    """SL.Ref with the instances in a term's visibility: _technique is SL's (the same statements; `occ` and `maybe` are extended)"""

    def _technique(self, k, j, T, L, n, S):
        c = self.case
        ii = np.nonzero(~T.no)[0]
        maybe_live = ~T.no
        self.traced_yes[k, j], self.traced_maybe[k, j] = T.yes.reshape(n, S), maybe_live.reshape(n, S)
        if not ii.size:
            return
        org = np.repeat(c.pos[L].astype(F64), S, 0)[ii]
        rr = TC.RayRef(c.geo, org, T.d[ii], T.bd[ii])
        with np.errstate(invalid="ignore"):
            occ = (rr.has & (rr.c["robust"] > 0) & (rr.t + rr.bt < c.t_max)).any(1)
            maybe = (rr.has & (rr.t - rr.bt < c.t_max)).any(1) | rr.overflow
        self.n_overflow += int(rr.overflow.sum())
        occ_o, maybe_o, over = instance_classes(c, np.repeat(c.pos[L], S, 0)[ii], T.d[ii], T.bd[ii])
        self.n_overflow += over
        occ, maybe = occ | occ_o, maybe | maybe_o
        vis = ~maybe
        sure = T.yes[ii]
        t, hi = T.t[ii], T.hi[ii]
        f = lambda a: a.reshape(n * S)
        lo_, hi_, mid_ = f(self.lo[k, j]), f(self.hi[k, j]), f(self.mid[k, j])
        lo_[ii] = np.where(vis & sure, np.maximum(T.lo[ii], 0.0), 0.0)
        hi_[ii] = np.where(occ, 0.0, hi)
        mid_[ii] = np.where(occ, 0.0, np.maximum(t, 0.0))
        self.lo[k, j], self.hi[k, j], self.mid[k, j] = lo_.reshape(n, S), hi_.reshape(n, S), mid_.reshape(n, S)
        vy, vm, un = f(self.vis_yes[k, j]), f(self.vis_maybe[k, j]), f(self.uncertain[k, j])
        vy[ii], vm[ii] = vis & sure, ~occ
        un[ii] = ~occ & ~(vis & sure)
        self.vis_yes[k, j], self.vis_maybe[k, j], self.uncertain[k, j] = vy.reshape(n, S), vm.reshape(n, S), un.reshape(n, S)


def check(case, F, stats=None, sentinel=None):
    """LC.check (SL.check for a SpecCase) against the extended reference -> (failures, worst share of an interval)"""
    return (SL.check if isinstance(case, SpecCase) else LC.check)(case, F, stats, sentinel)


# ---- float32 restatement of the rule (CPU), with the mutants the check must reject ------------------------------------------------------------------------------------

MUTANTS = ("objects_ignored", "scene_ignored", "transposed", "no_translation", "translated_dir", "object_to_world", "world_space", "far_blocks", "sum_not_union")


def _matrix(case, j, mut):
    W = case.w2o[j].copy().reshape(3, 4)
    if mut == "transposed":
        W[:, :3] = W[:, :3].T.copy()
    if mut == "no_translation":
        W[:, 3] = 0
    if mut == "world_space":
        W = np.eye(3, 4, dtype=F32)
    if mut == "object_to_world":
        W = case.poses[j].astype(F32)
    return W


def segment_blocker(case, mut=None, occluded=None, prefilter=True, only=None):
    """-> f(org [R,3] f32, dir [R,3] f32) -> [R] bool: some instance blocks the segment inside (0, t_max).  occluded(j, o' [R,3], d' [R,3], t_max) -> [R] bool;
    default: OC.occluded_f32 over the occluder's triangles.  only: the instances asked (default: all)"""
    t_max = F32(np.inf) if mut == "far_blocks" else F32(case.t_max)
    if occluded is None:
        occluded = lambda j, o, d, tm: OC.occluded_f32(MC.occluder(case.occ[case.inst[j]]), o, d, 0.0, tm)

    def blocked(org, dr):
        out = np.zeros(len(org), bool)
        if mut == "objects_ignored":
            return out
        for j in (range(case.J) if only is None else only):
            W = _matrix(case, j, mut)
            if not np.isfinite(W).all():
                continue
            o, d = MC.point_f32(W, org), MC.dir_f32(W, dr)
            if mut == "translated_dir":
                d = (d + W[None, :, 3]).astype(F32)
            ask = np.ones(len(org), bool)
            if prefilter:
                g = MC.occluder(case.occ[case.inst[j]])
                tri = g.verts[g.tris.reshape(-1)]
                ask = MC.box_f32(tri.min(0), tri.max(0), o, d)
            idx = np.nonzero(ask & ~out)[0]                                        # (a lane already blocked takes no further step: the OR is the same)
            if idx.size:
                out[idx] = np.asarray(occluded(j, o[idx], d[idx], t_max)).astype(bool)
        return out
    return blocked


def lights_mesh_f32(case, mut=None, trace=None, occluded=None, prefilter=True, sentinel=SENTINEL):
    """-> (F [K,Nt] f32, stats [2]): LC.lights_f32's arithmetic, called as it is, with the segment's visibility extended: its `trace` answers a hit at
    t = -1 (below any t_max) where an instance blocks.  trace(org, dir) -> (t, pid): the scene's closest hit (default TC.trace_f32)"""
    if mut == "sum_not_union":
        # two overlapping instances counted twice: the light each object takes alone, subtracted one after the other
        F, st = lights_mesh_f32(case, "objects_ignored", trace, occluded, prefilter, sentinel)
        out = F.copy()
        for j in range(case.J):
            Fj, _ = _lights(case, None, trace, occluded, prefilter, sentinel, only=[j])
            out = (out - (F - Fj)).astype(F32)
        return out, st
    return _lights(case, mut, trace, occluded, prefilter, sentinel)


def _lights(case, mut, trace, occluded, prefilter, sentinel, only=None):
    scene = trace or (lambda o_, d_: TC.trace_f32(case.geo, o_, d_)[:2])
    blocked = segment_blocker(case, mut, occluded, prefilter, only)

    def both(org, dr):
        if mut == "scene_ignored":
            t, pid = np.full(len(org), np.inf, F32), np.full(len(org), -1, np.int64)
        else:
            t, pid = scene(org, dr)
        b = blocked(np.asarray(org, F32), np.asarray(dr, F32))
        return np.where(b, F32(-1), np.asarray(t, F32)), np.where(b, 0, np.asarray(pid))
    return LC.lights_f32(case, None, sentinel, both)


def spec_lights_mesh_f32(case, trace=None, occluded=None, prefilter=True, sentinel=SENTINEL):
    """the same extension of SL.spec_lights_f32 -> (R [K,P] f32, stats [2])"""
    scene = trace or (lambda o_, d_: TC.trace_f32(case.geo, o_, d_)[:2])
    blocked = segment_blocker(case, None, occluded, prefilter)

    def both(org, dr):
        t, pid = scene(org, dr)
        b = blocked(np.asarray(org, F32), np.asarray(dr, F32))
        return np.where(b, F32(-1), np.asarray(t, F32)), np.where(b, 0, np.asarray(pid))
    return SL.spec_lights_f32(case, None, sentinel, both)


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------------------------------------------
# the room is [0, 8] x [0, 3] x [0, 6]; LC's panel hangs at y = 2.55 over (4, 3), 1.2 x 0.9 wide, shining down; its sphere (r = 0.15) floats at (4, 1.8, 3)

TABLE = lambda: MC.TABLE_AT()                                                      # the table under both lights: its top at y = 0.7 .. 0.76
TRI_OVER = lambda: MC.pose((4.0, 1.2, 2.6))                                        # the 3 x 3 triangle, level, between the floor and both lights
SCALED_ROT = lambda: MC.pose((4.2, 1.0, 3.1), (1, 2, 0.5), 35.0, (1.6, 0.5, 1.1))  # a non-uniform scale with a rotation
ABOVE_PANEL = lambda: MC.pose((4.0, 2.85, 3.0), (0, 1, 0), 15.0, (2.0, 0.15, 2.0))  # a slab between the panel and the ceiling: behind the light
ICO_OVER = lambda: MC.ICO_AT(4.0, 1.2, 3.0)

_CASES = {}


def _room_case(name, n, lights, S, first=3):
    geo, pos, nrm, shift, v, _, _ = LC.room_inputs()
    ids = v[first::max(1, len(v) // n - 1)][:n]
    assert len(ids) == n
    return LC.Case(name, geo, pos, nrm, shift, ids, lights, S)


def _outside_box(lo, hi, pad=0.05):
    geo, pos, nrm, shift, v, _, _ = LC.room_inputs()
    p = pos[v]
    inside = ((p > np.asarray(lo) - pad) & (p < np.asarray(hi) + pad)).all(1)
    return v[~inside], v[((p > np.asarray(lo) + pad) & (p < np.asarray(hi) - pad)).all(1)]


def case(name):
    if name in _CASES:
        return _CASES[name]
    two = np.stack([LC.room_quad_record(), LC.room_sphere_record()])
    if name == "table":                                                            # 200 texels, S = 64, quad and sphere, the table between floor and lights
        c = Case(name, LC.case("list200"), ["table"], [0], [TABLE()])
    elif name == "tri":                                                            # 63 shuffled texels, S = 17, a single triangle
        c = Case(name, LC.case("list63"), ["tri"], [0], [TRI_OVER()])
    elif name == "cube":                                                           # 63 texels, the cube scaled non-uniformly and rotated
        c = Case(name, LC.case("list63"), ["cube"], [0], [SCALED_ROT()])
    elif name == "one_sample":                                                     # 64 texels, S = 1, the panel alone (IEEE arithmetic), table and triangle
        c = Case(name, _room_case("q64", 64, two[:1], 1), ["table", "tri"], [0, 1], [TABLE(), TRI_OVER()])
    elif name == "one_sample_200":                                                 # the same question on 200 texels: more than one block of waves
        c = Case(name, _room_case("q200", 200, two[:1], 1, 5), ["table", "cube"], [0, 1], [TABLE(), SCALED_ROT()])
    elif name == "twice":                                                          # 65 texels, S = 2, two instances of one occluder, overlapping
        c = Case(name, LC.case("list65"), ["ico"], [0, 0], [ICO_OVER(), MC.ICO_AT(4.2, 1.3, 3.1, 70.0)])
    elif name == "s24":                                                            # 130 texels, S = 24: no power of two
        c = Case(name, _room_case("s24", 130, two, 24), ["table", "ico"], [0, 1], [MC.TABLE_AT(3.6, 2.8), MC.ICO_AT(4.6, 1.3, 3.3)])
    elif name == "eight":                                                          # K = 8 lights (refused records among them), J = 8 instances
        inst, poses = MC.eight_instances()
        poses = poses.copy()
        poses[0], poses[2] = ICO_OVER(), MC.pose((4.4, 0.9, 2.7), (0, 1, 0), 30.0)
        c = Case(name, LC.case("room_eight"), ["ico", "cube"], inst, poses)
    elif name == "null":                                                           # texel_ids NULL: all 200 texels of a compacted G-buffer
        c = Case(name, LC.case("null200"), ["table"], [0], [TABLE()])
    elif name == "none":                                                           # J = 0
        c = Case(name, LC.case("list1"), [], [], np.zeros((0, 3, 4)))
    elif name == "none200":
        c = Case(name, LC.case("list200"), ["table"], [], np.zeros((0, 3, 4)))
    elif name == "below":                                                          # far from every segment
        c = Case(name, LC.case("list65"), ["cube", "ico"], [0, 1], [MC.BELOW(), MC.pose((-2.0, -4.0, -2.5))])
    elif name == "below200":
        c = Case(name, LC.case("list200"), ["cube", "ico"], [0, 1], [MC.BELOW(), MC.pose((-2.0, -4.0, -2.5))])
    elif name == "nonfinite":                                                      # every matrix non-finite: the table stands under the lights and never blocks
        w = MC.to_world_to_object(np.stack([TABLE(), ICO_OVER()]))
        w[0, 7], w[1, 0] = np.nan, np.inf
        c = Case(name, LC.case("list63"), ["table", "ico"], [0, 1], w2o=w)
    elif name == "behind_light":                                                   # an object behind the panel, seen from the floor: beyond the sample point
        c = Case(name, LC.case("list63"), ["cube"], [0], [ABOVE_PANEL()])
    elif name == "enclosed":                                                       # a small sphere light inside MC.enclosing_cube, every listed texel outside
        out_ids, _ = _outside_box([2.5, -0.5, 1.75], [5.5, 0.5, 4.25])
        geo, pos, nrm, shift, _, _, _ = LC.room_inputs()
        base = LC.Case("enc", geo, pos, nrm, shift, out_ids[4::len(out_ids) // 190][:190], LC.sphere([4.0, 0.25, 3.0], 0.1)[None], 16)
        c = Case(name, base, ["cube"], [0], [MC.enclosing_cube()])
    elif name == "inside_box":                                                     # the texel list inside the occluder's box: the panel is shut out, the inner sphere is seen
        _, in_ids = _outside_box([2.5, -0.5, 1.75], [5.5, 0.5, 4.25])
        geo, pos, nrm, shift, _, _, _ = LC.room_inputs()
        base = LC.Case("inb", geo, pos, nrm, shift, in_ids[:70], np.stack([LC.room_quad_record(), LC.sphere([4.0, 0.25, 3.0], 0.1)]), 16)
        c = Case(name, base, ["cube"], [0], [MC.enclosing_cube()])
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


ALL = ("table", "tri", "cube", "one_sample", "one_sample_200", "twice", "s24", "eight", "null", "none", "below", "nonfinite", "behind_light", "enclosed", "inside_box")
# the cases whose objects must change nothing, with the LC case whose bits they must return
IDENTITIES = ("none", "none200", "nonfinite", "below", "below200")
ONE_SAMPLE = ("one_sample", "one_sample_200")
MUTANT_CASES = {"objects_ignored": "tri", "scene_ignored": "tri", "transposed": "cube", "no_translation": "tri", "translated_dir": "tri",
                "object_to_world": "cube", "world_space": "tri", "far_blocks": "behind_light", "sum_not_union": "twice"}


def spec_case(name):
    key = "spec:" + name
    if key in _CASES:
        return _CASES[key]
    if name == "table":                                                            # 63 shuffled pixels, S = 16
        c = SpecCase(name, SL.case("list63"), ["table"], [0], [TABLE()])
    elif name == "table200":                                                       # 200 pixels, S = 64
        c = SpecCase(name, SL.case("list200"), ["table"], [0], [TABLE()])
    elif name == "cube":                                                           # 63 shuffled pixels, S = 16
        c = SpecCase(name, SL.case("list63"), ["cube"], [0], [SCALED_ROT()])
    elif name == "twice":                                                          # 65 pixels, S = 100: no power of two
        c = SpecCase(name, SL.case("list65"), ["ico"], [0, 0], [ICO_OVER(), MC.ICO_AT(4.2, 1.3, 3.1, 70.0)])
    elif name == "one":                                                            # 64 pixels, S = 1
        c = SpecCase(name, SL.case("list64"), ["table", "tri"], [0, 1], [TABLE(), TRI_OVER()])
    elif name == "eight":                                                          # K = 8 lights, J = 8 instances
        c = SpecCase(name, SL.case("room_eight"), ["ico", "cube"], case("eight").inst, case("eight").poses)
    elif name == "dup_outside":                                                    # duplicates and ids outside the image
        c = SpecCase(name, SL.case("dup_outside"), ["tri"], [0], [TRI_OVER()])
    elif name == "none":
        c = SpecCase(name, SL.case("list200"), ["table"], [], np.zeros((0, 3, 4)))
    elif name == "below":
        c = SpecCase(name, SL.case("list200"), ["cube", "ico"], [0, 1], [MC.BELOW(), MC.pose((-2.0, -4.0, -2.5))])
    elif name == "nonfinite":
        c = SpecCase(name, SL.case("list200"), ["table", "ico"], [0, 1], w2o=case("nonfinite").w2o)
    else:
        raise KeyError(name)
    _CASES[key] = c
    return c


SPEC_ALL = ("table", "table200", "cube", "twice", "one", "eight", "dup_outside")
SPEC_IDENTITIES = ("none", "below", "nonfinite")
