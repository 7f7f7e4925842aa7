"""Cases of the specular shadow pass (include/texir_hip.h texir_spec_shadow, csrc/specshadow.hip): the float64 reference, the check of a result against it,
a float32 restatement of the rule with the mutants the check must reject, and the seeded cases.  Shared by test_spec_shadow_ref_cpu.py (no GPU) and
test_gpu_spec_shadow.py; no tests here.  Nothing is derived anew: the reference COMBINES the existing ones, none of which is changed.

  spec_cases              the GGX sample chain per sample: the weight w with its bound, the direction l with its per-component bound e, the admissible
                          branch variants at kinks (every (variant, sample) pair is one ray), MAX_UNC / CAP_LEFT_OUT, n_acc (the accumulation depth)
  trace_cases.RayRef      the candidate closest hits of a ray (x, l +- e) with t +- bound_t and the radiance interval; CAP_MULTI
  irt_shadow_cases.body64 a body's met / not met / uncertain status and t_b +- dt_b for the ray (x, l +- e): the header's body bound with e_i = the chain's bound
  irt_shadow_mesh_cases   the object-space ray (o' in the rule's float32 sequence, d' with the header's bound), box_classes for the prefilter's counts, and the
                          instance classification through occlusion_cases.classify_rayref
KF = 4, U = 2^-24 and TINY are texture_cases'; nothing is taken from a kernel's output.

PER SAMPLE AND SET.  Against closest-hit candidate c (distance t_s +- bound_t) member k of a set (bit k = body k, bit 8 + j = instance j) is certainly
BLOCKING (a body: certainly met and t_b + dt_b < t_s - bound_t; an instance: certainly occluded inside (0, t_s - bound_t)), certainly CLEAR, or uncertain.  A
set blocks c certainly if some member does, is clear if every member is, else uncertain: the outcome's interval is [w] * [L_c], [0, 0], or the hull of both.
A sample's interval is the hull over its admissible outcomes and variants.  A PIXEL's value must lie in (1 / S) times the sum of its samples' intervals,
widened by KF U n_acc(S, lpp) times the sum of the intervals' magnitudes (spec_cases.n_acc: the product, one addition per pass and shuffle level, the
division).  A pixel with a left-out sample (more than MAX_UNC uncertain kinks) is not compared.
stats must lie between certain and possible counts over the LIST (a duplicate counts again, an id outside [0, P) never): [0] samples whose ray meets a body
or a padded box; [1] occluder queries: at most one per (instance whose box is possibly met, possibly accepted hit); at least those of samples no body can be
in front of (a sample a body blocks may skip instances, see the header); [2] blocked samples.
CAPS (conditions on the reference alone, asserted per case in test_spec_shadow_ref_cpu.py): no candidate-list overflow; left-out samples at most
spec_cases.CAP_LEFT_OUT; rays with several candidate hits at most trace_cases.CAP_MULTI of those that may meet anything; pixels with an uncertain blocked
decision at most spec_light_cases.CAP_UNCERTAIN_PIXELS of the listed pixels.
"""
import math

import numpy as np

import irt_shadow_cases as SH
import irt_shadow_mesh_cases as MC
import occlusion_cases as OC
import spec_cases as SC
import spec_light_cases as SL
import trace_cases as TC
from texture_cases import K as KF, TINY, U

F32, F64 = np.float32, np.float64
SENTINEL = 7.0
CAP_LEFT_OUT = SC.CAP_LEFT_OUT
CAP_MULTI = TC.CAP_MULTI
CAP_UNCERTAIN_PIXELS = SL.CAP_UNCERTAIN_PIXELS
ROUGHNESS = SL.ROUGHNESS
MUTANTS = ("far_ignored", "one_sided", "shell", "sum_sets", "inst_bits_low", "high_bits", "no_weight", "ndl_weight", "no_over_S", "world_space", "add_missed")


def named_bits(Kb, J):
    return ((1 << Kb) - 1) | (((1 << J) - 1) << 8)


class Case:
    """pos, nrm [P,3], rough [P], shift [P,2] f32 of the whole pixel grid, cam [3]; ids: the listed pixels (duplicates and ids outside [0, P) allowed);
    bodies [Kbuf,16] f32 of which the first Kb are the call's; occ: names of the Q occluders; inst: occluder index per instance of the BUFFER, of which the
    first J are the call's; poses [Jbuf,3,4] object-to-world (or w2o [Jbuf,12] given directly); sets: M raw uint32 masks; lpp: TEXIR_SPEC_LPP (0: automatic)"""

    def __init__(self, name, geo, pos, nrm, rough, shift, cam, ids, S, bodies=(), occ=(), inst=(), poses=None, sets=(0xFFFFFFFF,), Kb=None, J=None, ceps=1e-14, lpp=0,
                 w2o=None, grid_cap=0):
        self.name, self.geo = "spec_shadow:" + name, geo
        self.pos, self.nrm = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.P = self.pos.shape[0]
        self.rough = np.ascontiguousarray(rough, F32).reshape(self.P)
        self.shift = np.ascontiguousarray(shift, F32).reshape(self.P, 2)
        self.cam = np.asarray(cam, F32).reshape(3)
        self.ids = np.ascontiguousarray(ids, np.int32)
        self.S, self.ceps, self.lpp, self.grid_cap = int(S), float(ceps), int(lpp), int(grid_cap)
        self.buf = np.ascontiguousarray(np.asarray(bodies, F32).reshape(-1, 16))
        self.Kb = len(self.buf) if Kb is None else int(Kb)
        self.bodies = self.buf[:self.Kb]
        self.occ = list(occ)
        self.inst_buf = [int(i) for i in inst]
        if w2o is not None:
            self.w2o_buf = np.ascontiguousarray(w2o, F32).reshape(-1, 12)
            self.poses_buf = None
        else:
            self.poses_buf = np.zeros((0, 3, 4)) if poses is None else np.asarray(poses, F64).reshape(-1, 3, 4)
            self.w2o_buf = MC.to_world_to_object(self.poses_buf) if len(self.inst_buf) else np.zeros((0, 12), F32)
        self.J = len(self.inst_buf) if J is None else int(J)
        self.inst, self.w2o = self.inst_buf[:self.J], self.w2o_buf[:self.J]
        self.poses = None if self.poses_buf is None else self.poses_buf[:self.J]
        self.sets = [int(s) & 0xFFFFFFFF for s in sets]
        self.M = len(self.sets)
        self.listed = np.unique(self.ids[(self.ids >= 0) & (self.ids < self.P)].astype(np.int64))
        self._ref = None

    def masks(self):
        return [s & named_bits(self.Kb, self.J) for s in self.sets]

    def geos(self):
        return [MC.occluder(n) for n in self.occ]

    def inputs(self, dtype=None):
        """spec_cases.sample_inputs of the listed pixels (what spec_cases.chain_f32 and reference take)"""
        import torch
        L = self.listed
        return SC.sample_inputs(self.nrm[L], self.rough[L], self.pos[L], self.cam, self.shift[L], self.S, torch.float64 if dtype is None else dtype)

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref


class Ref:
    def __init__(self, case):
        self.case = c = case
        L = self.pix = c.listed
        self.row_of = {int(t): i for i, t in enumerate(L)}
        S, P = c.S, len(L)
        names = ("w", "l0", "l1", "l2")
        if P == 0:
            self.left = np.zeros((0, S), bool)
            self.lo = self.hi = self.mid = [np.zeros((0, S, 3)) for _ in range(c.M)]
            self.overflow = 0
            z = np.zeros((0, S), bool)
            self.meet_yes = self.meet_maybe = self.blk_yes = self.blk_maybe = self.uncertain = self.multi = z
            self.q_yes = self.q_maybe = np.zeros((0, S), np.int64)
            self.spec_lo = self.spec_hi = np.zeros((0, S, 3))
            self.accepted_sure = z
            return
        dref = self.dref = SC.reference(c.inputs(), c.ceps, "spec", names)
        self.left = dref.left.reshape(P, S)
        vi, si = np.nonzero(dref.adm)                                            # (variant, sample) pairs: one ray each
        self.sample_of, self.variant_of = si, vi
        d = np.stack([dref.val[k][vi, si] for k in names[1:]], 1)
        bd = np.stack([dref.bnd[k][vi, si] for k in names[1:]], 1)               # KF included
        w, bw = dref.val["w"][vi, si], dref.bnd["w"][vi, si]
        x32 = c.pos[L][si // S]
        rays = self.rays = TC.RayRef(c.geo, x32.astype(F64), d, bd, 8)
        lo, hi, val, ok = rays.outcomes()                                        # [R, C + 1, 3]; the last slot is the zero outcome
        w_lo, w_hi = (w - bw)[:, None, None], (w + bw)[:, None, None]
        prod = [lo * w_lo, lo * w_hi, hi * w_lo, hi * w_hi]
        o_lo, o_hi = np.minimum.reduce(prod), np.maximum.reduce(prod)
        o_val = val * w[:, None, None]
        R, C1 = ok.shape
        C = C1 - 1
        with np.errstate(invalid="ignore"):
            t_lo, t_hi, t_s = rays.t - rays.bt, rays.t + rays.bt, rays.t          # [R, C]
        Kb, J = c.Kb, c.J
        NB = 16
        blocked = np.zeros((NB, R, C), bool)
        clear = np.ones((NB, R, C), bool)
        front64 = np.zeros((NB, R, C), bool)
        m_yes, m_maybe = np.zeros((NB, R), bool), np.zeros((NB, R), bool)
        self.overflow = int(rays.overflow.sum())
        for k in range(Kb):
            B = SH.body64(x32, d, bd / KF, c.bodies[k])
            m_yes[k], m_maybe[k] = B["yes"], ~B["no"]
            with np.errstate(invalid="ignore"):
                blocked[k] = B["yes"][:, None] & (B["tb_hi"][:, None] < t_lo)
                clear[k] = B["no"][:, None] | (B["tb_lo"][:, None] > t_hi)
                front64[k] = B["meets"][:, None] & (B["tb"][:, None] < t_s)
        geos = c.geos()
        for j in range(J):
            k = 8 + j
            if not np.isfinite(c.w2o[j]).all():
                continue                                                         # a matrix with a non-finite entry never blocks and meets nothing
            g = geos[c.inst[j]]
            W = c.w2o[j].astype(F64).reshape(3, 4)
            o32 = MC.point_f32(c.w2o[j], x32).astype(F64)
            d_o = d @ W[:, :3].T
            bd_o = bd @ np.abs(W[:, :3]).T + KF * (3 * U * (np.abs(d) @ np.abs(W[:, :3]).T) + 3 * TINY)
            tri = g.verts[g.tris.reshape(-1)]
            m_yes[k], m_maybe[k] = MC.box_classes(tri.min(0), tri.max(0), o32, d_o, bd_o)
            sel = np.nonzero(m_maybe[k])[0]
            rr = TC.RayRef(g, o32[sel], d_o[sel], bd_o[sel])
            self.overflow += int(rr.overflow.sum())
            for cc in range(C):
                occ_, _ = OC.classify_rayref(rr, t_lo[sel, cc][:, None])
                _, vis = OC.classify_rayref(rr, t_hi[sel, cc][:, None])
                blocked[k][sel, cc] = occ_
                clear[k][sel, cc] = vis
                with np.errstate(invalid="ignore"):
                    front64[k][sel, cc] = (rr.has & (rr.c["robust"] > 0) & (rr.t > 0) & (rr.t < t_s[sel, cc][:, None])).any(1)
        cand_ok = ok[:, :C]

        def per_sample(x_, fn, init):
            out = np.full((P * S,) + x_.shape[1:], init, x_.dtype)
            fn.at(out, si, x_)
            return out.reshape((P, S) + x_.shape[1:])
        base = np.nonzero(vi == 0)[0]
        first = ok[base].argmax(1)
        z = np.zeros((R, 1), bool)
        self.lo, self.hi, self.mid = [], [], []
        for mask in c.masks():
            ks = [k for k in range(NB) if mask >> k & 1]
            bl = blocked[ks].any(0) if ks else np.zeros((R, C), bool)
            cl = clear[ks].all(0) if ks else np.ones((R, C), bool)
            fr = front64[ks].any(0) if ks else np.zeros((R, C), bool)
            bl3, cl3 = np.concatenate([bl, z], 1)[..., None], np.concatenate([cl, ~z], 1)[..., None]
            s_lo = np.where(bl3, o_lo, np.where(cl3, 0.0, np.minimum(o_lo, 0.0)))
            s_hi = np.where(bl3, o_hi, np.where(cl3, 0.0, np.maximum(o_hi, 0.0)))
            r_lo = np.where(ok[..., None], s_lo, np.inf).min(1)
            r_hi = np.where(ok[..., None], s_hi, -np.inf).max(1)
            self.lo.append(per_sample(r_lo, np.minimum, np.inf))
            self.hi.append(per_sample(r_hi, np.maximum, -np.inf))
            v = np.where(np.concatenate([fr, z], 1)[..., None], o_val, 0.0)
            mid = np.zeros((P * S, 3))
            mid[si[base]] = v[base, first]
            self.mid.append(mid.reshape(P, S, 3))
        # the whole specular term's intervals (every accepted sample added): what lost is bounded by
        self.spec_lo = per_sample(np.where(ok[..., None], o_lo, np.inf).min(1), np.minimum, np.inf)
        self.spec_hi = per_sample(np.where(ok[..., None], o_hi, -np.inf).max(1), np.maximum, -np.inf)
        # counts per sample over every valid body and instance, whatever the sets
        acc_yes = ~ok[:, C] & cand_ok.any(1)
        acc_maybe = cand_ok.any(1)
        meet_yes, meet_maybe = m_yes.any(0), m_maybe.any(0)
        any_bl, all_cl = blocked.any(0), clear.all(0)
        body_clear = clear[:8].all(0)                                            # no body can be in front of candidate c
        no_body = np.where(cand_ok, body_clear, True).all(1)
        blk_yes = ~ok[:, C] & np.where(cand_ok, any_bl, True).all(1) & cand_ok.any(1)
        blk_maybe = (cand_ok & ~all_cl).any(1)
        unc_ray = meet_maybe & (cand_ok & ~any_bl & ~all_cl).any(1)               # the blocked decision of some admissible hit is open
        self.meet_yes = per_sample(meet_yes, np.logical_and, True)               # [P, S]: every variant
        self.meet_maybe = per_sample(meet_maybe, np.logical_or, False)
        self.q_yes = sum(per_sample(m_yes[8 + j] & acc_yes & no_body, np.logical_and, True).astype(np.int64) for j in range(8))
        self.q_maybe = sum(per_sample(m_maybe[8 + j] & acc_maybe, np.logical_or, False).astype(np.int64) for j in range(8))
        self.blk_yes = per_sample(blk_yes, np.logical_and, True)
        self.blk_maybe = per_sample(blk_maybe, np.logical_or, False)
        self.uncertain = per_sample(unc_ray, np.logical_or, False)
        self.multi = per_sample(meet_maybe & (rays.n_outcomes() > 1), np.logical_or, False)
        self.accepted_sure = per_sample(acc_yes, np.logical_and, True)
        for a in ("meet_yes", "q_yes", "blk_yes"):                               # a left-out sample is certain of nothing
            setattr(self, a, np.where(self.left, 0, getattr(self, a)).astype(getattr(self, a).dtype))

    def caps(self):
        """(candidate-list overflows, share of left-out samples, share of multi-candidate rays among the samples that may meet anything, share of the listed
        pixels with an uncertain blocked decision)"""
        n = max(self.left.size, 1)
        return (self.overflow, float(self.left.sum()) / n, float(self.multi.sum()) / max(int(self.meet_maybe.sum()), 1),
                float(self.uncertain.any(1).sum()) / max(len(self.pix), 1))

    def rows(self):
        ids = self.case.ids
        return np.array([self.row_of[int(t)] for t in ids if 0 <= t < self.case.P], np.int64)

    def counts(self):
        """over the LIST: [(lo, hi)] of stats[0], [1], [2]; a left-out sample may count anything it could"""
        rows = self.rows()
        g = lambda a: int(np.asarray(a)[rows].sum()) if len(rows) else 0
        lf = self.left
        return [(g(self.meet_yes), g(self.meet_maybe | lf)), (g(self.q_yes), g(np.where(lf, self.case.J, self.q_maybe))), (g(self.blk_yes), g(self.blk_maybe | lf))]

    def all_blocked(self, m):
        """[P] bool: every sample of the pixel has, for set m, exactly the whole specular term's interval, is certain of its hit, and some sample adds
        something: the pixels on which lost[m] must equal the specular term bit for bit"""
        same = ((self.lo[m] == self.spec_lo) & (self.hi[m] == self.spec_hi)).all(2)
        certain = ~self.uncertain & ~self.left
        return (same & certain).all(1) & (np.abs(self.mid[m]).sum((1, 2)) > 0)


RATIOS = {}


def check(case, lost, stats=None, sentinel=None, what=""):
    """lost [M, P, 3]: every listed pixel of every set inside its interval, unlisted pixels keep `sentinel`, stats inside its counts -> the worst
    error / bound; raises AssertionError naming what fails"""
    ref = case.ref()
    lost = np.asarray(lost, F64).reshape(case.M, case.P, 3)
    fails, worst = [], 0.0
    got_all = lost[:, ref.pix]
    skip = ref.left.any(1)
    if not np.isfinite(got_all[:, ~skip]).all():
        fails.append("non-finite values")
    nr = SC.n_acc(case.S, case.lpp)
    for m in range(case.M):
        lo_s, hi_s = ref.lo[m], ref.hi[m]
        with np.errstate(invalid="ignore"):
            LO, HI = lo_s.sum(1), hi_s.sum(1)
            mag = np.maximum(np.abs(lo_s), np.abs(hi_s)).sum(1)
            acc = KF * (nr * U * mag + (nr + 4) * TINY)
            lo, hi = (LO - acc) / case.S, (HI + acc) / case.S
        mid = ref.mid[m].sum(1) / case.S
        got = got_all[m]
        zero = (LO == 0) & (HI == 0) & (mag == 0) & ~skip[:, None]
        if (got[zero] != 0).any() or np.signbit(got[zero]).any():
            fails.append("set %d: %d values of pixels no sample of which can be blocked are not +0" % (m, int((got[zero] != 0).sum())))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(got >= mid, np.where(got == mid, 0.0, (got - mid) / (hi - mid)), (mid - got) / (mid - lo))
        ratio = np.where(zero | skip[:, None], 0.0, ratio)
        bad = ~(ratio <= 1.0)
        for i, ch in np.argwhere(bad)[:6]:
            fails.append("set %d pixel %d channel %d: %.9g outside [%.9g, %.9g] (reference %.9g)" % (m, ref.pix[i], ch, got[i, ch], lo[i, ch], hi[i, ch], mid[i, ch]))
        if bad.sum() > 6:
            fails.append("... set %d: %d values outside in all" % (m, int(bad.sum())))
        if ratio.size and not bad.any():
            worst = max(worst, float(ratio.max()))
    if sentinel is not None:
        un = np.setdiff1d(np.arange(case.P), ref.pix)
        if un.size and not (lost[:, un] == sentinel).all():
            fails.append("unlisted pixels were written")
    if stats is not None:
        s = [int(v) for v in np.asarray(stats).reshape(-1)[:3]]
        for i, (a, b) in enumerate(ref.counts()):
            if not a <= s[i] <= b:
                fails.append("stats[%d] = %d outside [%d, %d]" % (i, s[i], a, b))
    print("error/bound spec_shadow %-40s %s" % (case.name + " " + what, "rejected" if fails else "%.4f" % worst))
    if fails:
        raise AssertionError("%s %s:\n%s" % (case.name, what, "\n".join(fails)))
    RATIOS[case.name] = max(RATIOS.get(case.name, 0.0), worst)
    return worst


def rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


# ---- float32 restatement of the rule (CPU), op by op, with the mutants the check must reject ------------------------------------------------------------------------

_CHAIN, _TRACED, _LEAF = {}, {}, {}


def chain_f32(case):
    """(w [R] f32, l [R,3] f32) of the listed pixels' samples: spec_cases.chain_f32, the chain op by op in float32"""
    if case.name not in _CHAIN:
        if len(case.listed) == 0:
            _CHAIN[case.name] = (np.zeros(0, F32), np.zeros((0, 3), F32))
        else:
            w, _, l = SC.chain_f32(case, dual=True)
            _CHAIN[case.name] = (w.astype(F32), l.astype(F32))
    return _CHAIN[case.name]


def reduce_f32(terms, take, S, lpp):
    """the header's REDUCTION before the division: terms = (L [P,S,3], w [P,S]) f32, take [P,S] bool -> [P,3] f32.  Lane sl adds L * w (one fused
    multiply-add, as the kernel's contracted expression compiles) over the passes in ascending order; a sample not taken adds nothing; then the xor
    butterfly over the pixel's lanes"""
    L, w = terms
    P = L.shape[0]
    passes = (S + lpp - 1) // lpp
    acc = np.zeros((P, lpp, 3), F32)
    for q in range(passes):
        i = q * lpp + np.arange(lpp)
        ok = i < S
        ii = np.where(ok, i, 0)
        Lq, wq, tq = L[:, ii].astype(F64), w[:, ii].astype(F64), take[:, ii] & ok[None]
        with np.errstate(all="ignore"):
            new = (Lq * wq[..., None] + acc.astype(F64)).astype(F32)
        acc = np.where(tq[..., None], new, acc)
    o = lpp >> 1
    while o:
        with np.errstate(all="ignore"):
            acc = (acc + acc[:, np.arange(lpp) ^ o]).astype(F32)
        o >>= 1
    return acc[:, 0]


def object_rays(case, j, x, d, mut=None):
    W = case.w2o_buf[j].copy().reshape(3, 4)
    if mut == "world_space":
        W = np.eye(3, 4, dtype=F32)
    return W, MC.point_f32(W, x), MC.dir_f32(W, d)


def spec_shadow_f32(case, mut=None, trace=None, sentinel=SENTINEL, prefilter=True):
    """the header operation by operation -> (lost [M,P,3] f32, stats [3]); unlisted pixels hold the sentinel.  trace: None (brute force on the CPU:
    trace_cases.trace_f32 / shade_f32, occlusion_cases.leaf_f32) or an object with scene(org, dir) -> (t, pid, radiance [R,3]) and
    occluded(j, org, dir, t_far [R]) -> [R] bool: a device's own answers for the restated rays"""
    c = case
    L, S, P = c.listed, c.S, len(c.listed)
    w, l = chain_f32(c)
    x = np.repeat(c.pos[L], S, 0)
    R = P * S
    if trace is None:
        if c.name not in _TRACED:
            t, pid, uv = TC.trace_f32(c.geo, x, l) if R else (np.zeros(0, F32), np.zeros(0, np.int32), np.zeros((0, 2), F32))
            _TRACED[c.name] = (t, pid, TC.shade_f32(c.geo, t, pid, uv) if R else np.zeros((0, 3), F32))
        t, pid, rad = _TRACED[c.name]
    else:
        t, pid, rad = trace.scene(x, l)
    with np.errstate(invalid="ignore"):
        accepted = np.isfinite(t) & (t > F32(1e-4)) & (pid >= 0)
    far = np.full(R, np.inf, F32) if mut == "far_ignored" else np.where(accepted, t, F32(0)).astype(F32)
    high = mut == "high_bits"
    recs = c.buf if high else c.bodies
    n_inst = len(c.inst_buf) if high else c.J
    met, front = np.zeros((16, R), bool), np.zeros((16, R), bool)
    for k in range(min(len(recs), 8)):
        kind = SH.LC.record_kind(recs[k])
        if kind is None:
            continue
        met[k], tb = (SH.quad_f32 if kind == "quad" else SH.ball_f32)(recs[k], x, l, mut)
        with np.errstate(invalid="ignore"):
            front[k] = met[k] & (tb < far)
    geos = c.geos()
    queries = np.zeros(R, np.int64)
    for j in range(min(n_inst, 8)):
        W, o, dd = object_rays(c, j, x, l, mut)
        if not np.isfinite(W).all():
            continue
        g = geos[c.inst_buf[j]]
        tri = g.verts[g.tris.reshape(-1)]
        met[8 + j] = MC.box_f32(tri.min(0), tri.max(0), o, dd) if prefilter else True
        if trace is None:
            key = (c.name, j, mut == "world_space")
            if key not in _LEAF:
                _LEAF[key] = OC.leaf_f32(g, o, dd) if R else (np.zeros((0, g.T), bool), np.zeros((0, g.T), F32))
            inside, tt = _LEAF[key]
            with np.errstate(invalid="ignore"):
                hit = (inside & (tt > 0) & (tt < far[:, None])).any(1)
            assert not (hit & ~met[8 + j]).any(), "the prefilter rejects a ray the leaf test accepts"
        else:
            hit = np.asarray(trace.occluded(j, o, dd, far)).astype(bool) & met[8 + j]
        front[8 + j] = hit & accepted
        queries += met[8 + j] & accepted
    front &= accepted[None]
    take_all = mut == "add_missed"
    Lr = np.where(accepted[:, None], rad, F32(0)).astype(F32)
    wt = w
    if mut == "no_weight":
        wt = np.ones(R, F32)
    elif mut == "ndl_weight":
        n = np.repeat(c.nrm[L], S, 0)
        wt = np.clip((n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2], F32(0), F32(1)).astype(F32)
    lpp = SC.lanes_per_pixel(S, c.lpp)
    out = np.full((c.M, c.P, 3), sentinel, F32)
    for m, mask in enumerate(c.sets if high else c.masks()):
        if high:
            mask |= (mask >> 16) & 0xFFFF                                         # bits 16..31 honoured as aliases of 0..15
        if mut == "inst_bits_low":
            mask = (mask & 0xFF) | ((mask & 0xFF) << 8)                           # instances read from bits 0..7
        ks = [k for k in range(16) if mask >> k & 1]
        if mut == "sum_sets":
            cnt = front[ks].sum(0) if ks else np.zeros(R, np.int64)
            v = np.zeros((P, 3), F32)
            for rep in range(1, 17):                                              # a per-member sum: a sample in front of n members is added n times
                v = (v + reduce_f32((Lr.reshape(P, S, 3), wt.reshape(P, S)), (cnt >= rep).reshape(P, S), S, lpp)).astype(F32) if (cnt >= rep).any() else v
        else:
            take = (front[ks].any(0) if ks else np.zeros(R, bool))
            if take_all:
                take = accepted
            v = reduce_f32((Lr.reshape(P, S, 3), wt.reshape(P, S)), take.reshape(P, S), S, lpp)
        with np.errstate(all="ignore"):
            out[m, L] = v if mut == "no_over_S" else (v / F32(S)).astype(F32)
    rows = np.searchsorted(L, c.ids[(c.ids >= 0) & (c.ids < c.P)].astype(np.int64))
    mult = np.bincount(rows, minlength=P)
    g3 = lambda a: int((a.reshape(P, S) * mult[:, None]).sum()) if R else 0
    return out, np.array([g3(met.any(0)), g3(queries), g3(front.any(0))], np.int64)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------------------------

# the box is [0, 8] x [0, 3] x [0, 6] and so, within half a centimetre, is the room; pixels are the golden atlases' texels, 0.01 inside their faces
PANEL, BALL, OUTSIDE, FAR = SH.PANEL, SH.BALL, SH.OUTSIDE, SH.FAR
TABLE_AT, ICO_AT, BELOW = MC.TABLE_AT, MC.ICO_AT, MC.BELOW
COVER_BALL = lambda: SH.ball([4.0, 0.0, 3.0], 1.5)                                # around a patch of floor pixels: they are INSIDE it, t_b = 0
_CASES, _GRID = {}, {}


def cam():
    """spec_light_cases.room_cam() where it lies inside the golden box and room (it does: the two rooms share their extent within centimetres)"""
    v = SL.room_cam()
    assert (v > [0.5, 0.5, 0.5]).all() and (v < [7.5, 2.5, 5.5]).all(), v
    return v


def grid(scene):
    """(geo, pos, nrm, rough, shift, floor and wall pixel ids) of a golden atlas: every pixel one of the product's four roughness values"""
    if scene not in _GRID:
        geo, gb = TC.golden_geo(scene)
        pos, nrm = gb["pos"].reshape(-1, 3), gb["nrm"].reshape(-1, 3)
        shift = np.random.default_rng(77).random((len(pos), 2), dtype=F32)
        valid = gb["valid"].reshape(-1) > 0
        # floor and wall pixels the camera sees from their front side, away from the edges of their faces
        facing = ((cam()[None].astype(F64) - pos) * nrm).sum(1) > 0.2
        ok = valid & facing & (nrm[:, 1] > -0.5) & (np.abs(nrm).max(1) > 0.99)
        _GRID[scene] = (geo, pos, nrm, SL.room_rough(len(pos)), shift, np.nonzero(ok)[0])
    return _GRID[scene]


def spread(scene, n, first=0):
    v = grid(scene)[5]
    return v[first:: max(1, (len(v) - first) // n)][:n]


def toward(scene, centre, radius):
    """the pixels whose MIRROR ray (the camera's direction reflected about the raw normal: the lobe's axis) passes within `radius` of `centre`, ahead"""
    geo, pos, nrm, _, _, v = grid(scene)
    x, n = pos[v].astype(F64), nrm[v].astype(F64)
    vv = cam()[None].astype(F64) - x
    vv /= np.linalg.norm(vv, axis=1, keepdims=True)
    l = 2 * (n * vv).sum(1, keepdims=True) * n - vv
    q = np.asarray(centre, F64)[None] - x
    along = (q * l).sum(1)
    off = np.linalg.norm(q - along[:, None] * l, axis=1)
    return v[(along > 0) & (off < radius)]


def pool(scene, n, targets, first=0):
    """candidate pixels of a case, 4 n of them: alternately pixels whose mirror ray goes toward one of the targets [(centre, radius)] and pixels spread over
    the floor and the walls.  choose() takes the case's n from them"""
    near = [toward(scene, c, r) for c, r in targets]
    near = [a[first % max(len(a), 1):: max(1, len(a) // (2 * n))] for a in near if len(a)]
    far = spread(scene, 4 * n, first)
    out, seen, i = [], set(), 0
    lists = near + [far]
    while len(out) < 4 * n and any(i < len(a) for a in lists):
        for a in lists:
            if i < len(a) and int(a[i]) not in seen:
                seen.add(int(a[i]))
                out.append(int(a[i]))
        i += 1
    return np.array(out[:4 * n], np.int64)


def choose(make, candidates, n, unsure=0):
    """the first n candidate pixels on which the REFERENCE ALONE is sharp -- no left-out sample, no ray that may meet something with several candidate
    hits, no uncertain blocked decision -- so that the case stays inside every cap (a condition on the reference, not on any kernel's output).  unsure: so
    many of the n are instead the first candidates WITH an uncertain blocked decision (and nothing else open): the hulls of the reference then meet a
    result; the caller keeps unsure / n under CAP_UNCERTAIN_PIXELS"""
    r = make(candidates).ref()
    other = r.left.any(1) | r.multi.any(1)
    order = {int(t): i for i, t in enumerate(candidates)}
    first = lambda mask, k: sorted((int(t) for t in r.pix[mask]), key=lambda t: order[t])[:k]
    open_ = first(r.uncertain.any(1) & ~other, unsure)
    assert len(open_) == unsure, "%d pixels with an uncertain decision among %d candidates, %d wanted" % (len(open_), len(candidates), unsure)
    sharp = first(~(other | r.uncertain.any(1)), n - unsure)
    ids = np.array(sorted(sharp + open_, key=lambda t: order[t]), np.int64)
    assert len(ids) == n, "%d sharp pixels among %d candidates, %d wanted" % (len(sharp), len(candidates), n - unsure)
    return ids


def inside_ball(scene, rec, n=None, shrink=0.8):
    geo, pos, nrm, _, _, v = grid(scene)
    d2 = ((pos[v].astype(F64) - rec[1:4].astype(F64)) ** 2).sum(1)
    sel = v[d2 < (shrink * float(rec[4])) ** 2]
    return sel if n is None else sel[:n]


def enclosed(scene, n=None):
    """floor pixels well inside irt_shadow_mesh_cases.enclosing_cube()"""
    geo, pos, nrm, _, _, v = grid(scene)
    p = pos[v]
    sel = v[(nrm[v][:, 1] > 0.9) & (np.abs(p[:, 0] - 4.0) < 1.2) & (np.abs(p[:, 2] - 3.0) < 1.0) & (p[:, 1] < 0.3)]
    return sel if n is None else sel[:n]


def eight():
    inst, poses = MC.eight_instances()
    return dict(bodies=SH.eight_records(), occ=["ico", "cube"], inst=inst, poses=poses)


BACK_PANEL = lambda: SH.quad([3.0, 2.5, 2.0], [0.0, 0.0, 2.0], [2.0, 0.0, 0.0])      # PANEL with its edges swapped: a x b = (0, 4, 0), rays from below meet its BACK
TWO_ONE = lambda: dict(bodies=np.stack([BALL(), PANEL()]), occ=["table"], inst=[0], poses=[TABLE_AT(5.5, 2.0)])
THREE_TWO = lambda: dict(bodies=np.stack([PANEL(), BALL(), OUTSIDE()]), occ=["table", "ico"], inst=[0, 1], poses=[TABLE_AT(5.5, 2.0), ICO_AT(2.5, 1.0, 4.0)])
T_BALL, T_PANEL, T_TABLE, T_ICO = ((4.0, 1.25, 3.0), 0.4), ((4.0, 2.5, 3.0), 0.8), ((5.5, 0.5, 2.0), 0.5), ((2.5, 1.0, 4.0), 0.7)
B, I = lambda *k: sum(1 << i for i in k), lambda *j: sum(1 << (8 + i) for i in j)


def case(name):
    if name in _CASES:
        return _CASES[name]
    scene = "room" if name.startswith("room") else "box"
    geo, pos, nrm, rough, shift, _ = grid(scene)

    def mk(n, S, targets=(), first=0, candidates=None, g=geo, unsure=0, **kw):
        make = lambda ids: Case(name, g, pos, nrm, rough, shift, cam(), ids, S, **kw)
        return make(choose(make, pool(scene, n, targets, first) if candidates is None else candidates, n, unsure))
    if name.startswith("s1_p"):                                                    # S = 1 (lpp 1): P in 1, 63, 64, 65, 200; M = 1 .. 5 across them
        n = int(name[4:])
        M = {1: 1, 63: 2, 64: 3, 65: 4, 200: 5}[n]
        c = mk(n, 1, [T_BALL, T_PANEL, T_TABLE], 3, sets=[B(0, 1) | I(0), B(0), I(0), B(1), 0][:M], ceps=1e-6 if n % 2 else 1e-14, **TWO_ONE())
    elif name in ("s16_p3", "s16_p4", "s16_p5"):                                   # S = 16 (lpp 16: four pixels per wave)
        n = int(name[5:])
        c = mk(n, 16, [T_BALL, T_TABLE, T_ICO], 11, sets=[B(0, 1, 2) | I(0, 1), B(1), I(0), I(1) | B(0), 0, 0xFFFF0000, B(2), B(0, 1)][:{3: 2, 4: 4, 5: 8}[n]], **THREE_TWO())
    elif name == "s16_grid":                                                       # more pixel groups than waves of a grid of two blocks (TEXIR_SPEC_GRID_CAP=2)
        # two of its 103 pixels (under CAP_UNCERTAIN_PIXELS) hold a sample whose blocked decision the reference leaves open: a silhouette
        c = mk(4 * 3 * 8 + 7, 16, [T_BALL, T_PANEL, T_TABLE, T_ICO], 5, unsure=2, sets=[B(0, 1, 2) | I(0, 1), I(0, 1)], grid_cap=2, **THREE_TWO())
    elif name == "s64_p1":                                                         # Kb / J = (1, 0)
        c = mk(1, 64, [T_BALL], 2, bodies=BALL()[None], sets=[B(0)])
    elif name == "s64_p2":                                                         # Kb / J = (0, 1)
        c = mk(2, 64, [((4.0, 1.25, 3.0), 0.7)], 1, occ=["ico"], inst=[0], poses=[ICO_AT()], sets=[I(0)])
    elif name == "s24_eight":                                                      # one partial pass; Kb / J = (8, 8), M = 8: every kind of mask
        c = mk(20, 24, [((2.2, 1.1, 2.1), 0.7), ((5.5, 0.5, 1.5), 0.5), ((7.99, 1.5, 3.0), 0.8)], 7,
               sets=[B(0), B(1), B(0, 1), 0, 0xFFFFFF00, 0xFF, I(0, 1) | B(5), I(2, 3, 4, 5, 6, 7) | B(3, 7)], **eight())
    elif name == "s100":                                                           # two passes, the second partial
        c = mk(12, 100, [T_BALL, T_TABLE, T_ICO], 2, sets=[B(0, 1, 2) | I(0, 1), B(0) | I(1), I(0)], ceps=1e-6, **THREE_TWO())
    elif name.startswith("lpp"):                                                   # TEXIR_SPEC_LPP in 1, 4, 16 at S in 16, 24
        lpp, S = (int(v) for v in name[3:].split("_s"))
        c = mk(64 // lpp + 1 if lpp > 1 else 9, S, [T_BALL, T_TABLE, T_ICO], 9, sets=[B(0, 1, 2) | I(0, 1), B(1) | I(0)], lpp=lpp, **THREE_TWO())
    elif name == "none":                                                           # Kb = J = 0
        c = mk(65, 16, (), 1, sets=[0xFFFFFFFF])
    elif name == "tri":                                                            # the one-triangle occluder: its tree is a root leaf
        c = mk(30, 16, [((4.0, 1.5, 3.0), 1.0)], 3, occ=["tri"], inst=[0], poses=[MC.pose((4.0, 1.5, 3.0), (0, 0, 1), 10.0, 2.0)], sets=[I(0)])
    elif name == "twice":                                                          # one handle named twice, overlapping: the sets {0}, {1}, {0, 1}
        c = mk(30, 16, [((4.1, 1.3, 3.1), 0.8)], 4, occ=["ico"], inst=[0, 0], poses=[ICO_AT(), ICO_AT(4.3, 1.4, 3.2, 70.0)], sets=[I(0), I(1), I(0, 1)])
    elif name == "nan_matrix":                                                     # a matrix with a NaN never blocks; the other instance does
        w2o = MC.to_world_to_object(np.stack([ICO_AT(), TABLE_AT(5.5, 2.0)]))
        w2o[0, 5] = np.nan
        c = mk(30, 16, [T_TABLE, T_BALL], 4, occ=["ico", "table"], inst=[0, 1], w2o=w2o, sets=[I(0), I(1), I(0, 1)])
    elif name == "highbits":                                                       # Kb = 1 and J = 1 of buffers of two: the other bits name nothing of the call
        c = mk(40, 16, [T_BALL, T_TABLE], 6, bodies=np.stack([OUTSIDE(), BALL()]), occ=["ico", "table"], inst=[0, 1], poses=[BELOW(), TABLE_AT(5.5, 2.0)], Kb=1, J=1,
               sets=[B(0, 1) | I(0, 1), B(1) | I(1), 0x01020000 | B(1)])
    elif name == "far":                                                            # nothing any ray can be blocked by: bodies behind the walls, objects below
        c = mk(65, 16, [((-2.5, 1.5, 3.0), 1.0)], 2, bodies=np.stack([FAR(), OUTSIDE()]), occ=["cube", "ico"], inst=[0, 1], poses=[BELOW(), MC.pose((-2.0, -4.0, -2.5))],
               sets=[0xFFFF, B(0), I(0, 1)])
    elif name == "open_top":                                                       # above the open top: met only by rays that leave the scene
        c = mk(40, 16, [((4.0, 6.0, 3.0), 2.0)], 3, g=SH.box_open(), bodies=SH.ball([4.0, 6.0, 3.0], 2.5)[None], occ=["ico"], inst=[0], poses=[ICO_AT(4.0, 6.0, 3.0, 35.0, 3.0)],
               sets=[B(0) | I(0), B(0)])
    elif name == "back":                                                           # rays from below meet the panel's BACK: two-sided here
        c = mk(40, 16, [T_PANEL], 8, bodies=BACK_PANEL()[None], sets=[B(0)])
    elif name == "overlap":                                                        # a ball and an icosphere around the same place: the union counts a sample once
        c = mk(40, 16, [T_BALL], 8, bodies=BALL()[None], occ=["ico"], inst=[0], poses=[ICO_AT(4.0, 1.25, 3.0, 35.0, 0.6)], sets=[B(0) | I(0), B(0), I(0)])
    elif name == "in_ball":                                                        # pixels inside a ball body
        c = mk(12, 16, candidates=inside_ball("box", COVER_BALL()), bodies=COVER_BALL()[None], sets=[B(0)])
    elif name == "in_cube":                                                        # pixels inside a closed box that cuts through the floor
        c = mk(12, 16, candidates=enclosed("box"), occ=["cube"], inst=[0], poses=[MC.enclosing_cube()], sets=[I(0)])
    elif name == "room_person":                                                    # the room's 20 k triangles, the 1984-triangle object and the table
        c = mk(65, 16, [T_BALL, T_PANEL, ((4.0, 0.9, 3.0), 0.6), ((3.0, 0.5, 2.5), 0.5)], 5, bodies=np.stack([PANEL(), BALL()]), occ=["person", "table"], inst=[0, 1],
               poses=[MC.pose((4.0, 0.0, 3.0), (0, 1, 0), 40.0), TABLE_AT(3.0, 2.5)], sets=[B(0, 1) | I(0, 1), I(0), I(1)])
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


LPP_CASES = tuple("lpp%d_s%d" % (lpp, S) for lpp in (1, 4, 16) for S in (16, 24))
GPU_CASES = ("s1_p1", "s1_p63", "s1_p64", "s1_p65", "s1_p200", "s16_p3", "s16_p4", "s16_p5", "s16_grid", "s64_p1", "s64_p2", "s24_eight", "s100") + LPP_CASES + (
    "none", "tri", "twice", "nan_matrix", "highbits", "far", "open_top", "back", "overlap", "in_ball", "in_cube", "room_person")
CPU_CASES = ("s1_p65", "s16_p3", "s16_p5", "s16_grid", "s64_p2", "s24_eight", "s100", "lpp4_s24", "none", "tri", "twice", "nan_matrix", "highbits", "far", "open_top", "back", "overlap",
             "in_ball", "in_cube")
# where each mutant must be rejected
MUTANT_CASES = {"far_ignored": "far", "one_sided": "back", "shell": "in_ball", "sum_sets": "overlap", "inst_bits_low": "s16_p5", "high_bits": "highbits",
                "no_weight": "in_ball", "ndl_weight": "in_ball", "no_over_S": "in_cube", "world_space": "s16_p5", "add_missed": "overlap"}
