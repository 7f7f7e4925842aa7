"""Cases of the body-shadow pass (include/texir_hip.h texir_irt_shadow, csrc/irtshadow.hip): the float64 reference, the check of a result against it, a
float32 restatement of the rule with the mutants the check must reject, and the seeded cases.  Shared by test_irt_shadow_ref_cpu.py (no GPU) and
test_gpu_irt_shadow.py; no tests here.  Rays, candidate lists, radiance intervals and the direction chain come from trace_cases / spec_cases, the record
layout and its validity rule from light_cases; none of them is changed.  KF = 4, U = 2^-24 and TINY are texture_cases'; every margin below is the header's
ROUNDING BOUND times KF, fixed before any GPU run; nothing is taken from a kernel's output.

THE REFERENCE is trace_cases.IrtRef's per-sample outcomes (every admissible direction variant, every admissible closest-hit candidate with its distance
t_s +- bound_t and its radiance interval, the zero outcome where a miss or the cut t > 1e-4 admits it), each extended by the body tests in float64:
  body k against the ray (x, d +- e)    MEETS certainly / certainly not / uncertain: a test of the rule (t > 0, the parallelogram coordinates at 0 and 1,
                                        disc >= 0, the far root's sign) is decided only beyond KF times the header's bound of its quantity; a ray within
                                        its bound of parallel to a quad's plane is decided where the hit point provably lies more than twice the quad's
                                        reach away;  t_b in [tb_lo, tb_hi]
  body k against candidate c            certainly BLOCKED: meets certainly and tb_hi < t_s - bound_t;  certainly CLEAR: certainly no meeting, or
                                        tb_lo > t_s + bound_t;  else uncertain
  set m against candidate c             blocked if some body of the set certainly blocks, clear if every body of the set is certainly clear, else uncertain
  interval of the outcome               blocked: the outcome's own [lo, hi] (radiance interval x n.l interval);  clear: [0, 0];  uncertain: [min(lo, 0), max(hi, 0)]
A sample's interval is the hull over its admissible outcomes; lost[m] of a texel must lie inside (2 pi / N) times the sum of its samples' intervals,
widened by KF u n_acc(N, 'group', parts) sum |terms| as IrtRef.check widens.  stats[0] must lie between the count of certainly-meeting samples and that
plus the uncertain ones, stats[1] likewise for blocked samples (an accepted hit behind SOME body, whatever the sets), both over the LIST.
CAPS (from the reference alone, asserted in test_irt_shadow_ref_cpu.py): no ray overflows its candidate list; at most CAP_MULTI = 2 % of the samples that
may meet a body are uncertain in any of this.
"""
import math

import numpy as np

import light_cases as LC
import spec_cases as SC  # noqa: F401  (the direction chain behind IrtRef)
import trace_cases as TC
from texture_cases import K as KF, TINY, U

F32, F64 = np.float32, np.float64
CAP_MULTI = TC.CAP_MULTI
SENTINEL = 7.0
MAX_BODIES = MAX_SETS = 8


# ---- the body tests in float64, with the header's bounds (WITHOUT KF; the callers multiply) ---------------------------------------------------------------------

def quad_record_f32(rec):
    """what the rule derives from a quad's record alone, in its float32 operation sequence: (o, m, mm, ua, vb) -- the same bits on any IEEE machine"""
    rec = np.asarray(rec, F32)
    o, a, b = rec[1:4], rec[4:7], rec[7:10]
    with np.errstate(all="ignore"):
        m = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
        mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        ua = np.array([(b[1] * m[2] - b[2] * m[1]) / mm, (b[2] * m[0] - b[0] * m[2]) / mm, (b[0] * m[1] - b[1] * m[0]) / mm], F32)
        vb = np.array([(m[1] * a[2] - m[2] * a[1]) / mm, (m[2] * a[0] - m[0] * a[2]) / mm, (m[0] * a[1] - m[1] * a[0]) / mm], F32)
    return o, m, mm, ua, vb


def body64(x, d, e, rec):
    """x [R,3] float32 values, d, e [R,3] float64 (e: the bound of d, without KF); rec: one record -> dict of [R] arrays: yes / no (meets certainly /
    certainly not), meets and tb (the float64 decision and entry distance), tb_lo / tb_hi (KF included; meaningful unless `no`).  What depends on x and
    the record alone (m, mm, ua, vb, q, num; oc, rr, cc) is taken in the rule's float32 sequence, as the header's bound does"""
    R = len(x)
    kind = LC.record_kind(rec)
    out = dict(yes=np.zeros(R, bool), no=np.ones(R, bool), meets=np.zeros(R, bool), tb=np.zeros(R), tb_lo=np.zeros(R), tb_hi=np.zeros(R))
    if kind is None:
        return out
    x32 = np.asarray(x, F32)
    ad = np.abs(d)
    with np.errstate(all="ignore"):
        if kind == "quad":
            o, m, mm, ua, vb = quad_record_f32(rec)
            if not (np.isfinite(mm) and mm > 0):
                return out                                                       # the rule's extra refusal of a quad
            q32 = [o[i] - x32[:, i] for i in range(3)]
            num = ((m[0] * q32[0] + m[1] * q32[1]) + m[2] * q32[2]).astype(F64)
            q = np.stack(q32, 1).astype(F64)
            m, ua, vb = m.astype(F64), ua.astype(F64), vb.astype(F64)
            den = (d * m).sum(1)
            dden = 3 * U * (ad * np.abs(m)).sum(1) + (np.abs(m) * e).sum(1) + 3 * TINY
            t = num / den
            dt = np.abs(t) * dden / np.abs(den) + U * np.abs(t) + TINY
            h = t[:, None] * d - q
            dh = ad * dt[:, None] + np.abs(t)[:, None] * e + U * (np.abs(t[:, None] * d) + np.abs(h)) + TINY
            u, v = (h * ua).sum(1), (h * vb).sum(1)
            du = 3 * U * (np.abs(h) * np.abs(ua)).sum(1) + (np.abs(ua) * dh).sum(1) + 3 * TINY
            dv = 3 * U * (np.abs(h) * np.abs(vb)).sum(1) + (np.abs(vb) * dh).sum(1) + 3 * TINY
            decided = np.abs(den) > KF * dden                                    # the ray is not within its bound of the quad's plane direction
            inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
            out["meets"] = (den != 0) & np.isfinite(t) & (t > 0) & inside
            out["tb"] = np.where(out["meets"], t, 0.0)
            yes = decided & (t > KF * dt) & (u >= KF * du) & (u <= 1 - KF * du) & (v >= KF * dv) & (v <= 1 - KF * dv)
            no = decided & ((t < -KF * dt) | (u < -KF * du) | (u > 1 + KF * du) | (v < -KF * dv) | (v > 1 + KF * dv))
            # within its bound of parallel: any float32 t is at least t_min; a hit point that far lies outside the quad whatever its coordinates' roundings
            r64 = np.asarray(rec, F32).astype(F64)
            o_, a_, b_ = r64[1:4], r64[4:7], r64[7:10]
            corners = np.stack([o_, o_ + a_, o_ + b_, o_ + a_ + b_])
            reach = np.linalg.norm(corners[None] - x32.astype(F64)[:, None], axis=-1).max(1)
            t_min = np.abs(num) / (np.abs(den) + KF * dden)
            far_off = ~decided & (t_min * np.linalg.norm(d, axis=1) > 2 * reach + 1)
            out["yes"], out["no"] = yes, no | far_off | ~np.isfinite(d).all(1)
            out["tb_lo"], out["tb_hi"] = t - KF * dt, t + KF * dt
        else:
            r32 = np.asarray(rec, F32)
            c32, rad = r32[1:4], r32[4]
            rr = rad * rad
            oc32 = [c32[i] - x32[:, i] for i in range(3)]
            cc = (((oc32[0] * oc32[0] + oc32[1] * oc32[1]) + oc32[2] * oc32[2]) - rr).astype(F64)
            oc = np.stack(oc32, 1).astype(F64)
            aoc = np.abs(oc)
            b = (oc * d).sum(1)
            db = 3 * U * (aoc * ad).sum(1) + (aoc * e).sum(1) + 3 * TINY
            dd = (d * d).sum(1)
            ddd = 3 * U * dd + 2 * (ad * e).sum(1) + 3 * TINY
            disc = b * b - dd * cc
            ddisc = 2 * np.abs(b) * db + U * b * b + np.abs(cc) * ddd + U * np.abs(dd * cc) + U * np.abs(disc) + 3 * TINY
            sq = np.sqrt(np.maximum(disc, 0))
            lin = ddisc / (2 * np.sqrt(np.maximum(disc - ddisc, 0)))
            dsq = np.minimum(np.where(np.isfinite(lin), lin, np.inf), np.sqrt(ddisc)) + U * sq
            s = b + sq
            ds = db + dsq + U * np.abs(s) + TINY
            tb = np.where(cc <= 0, 0.0, cc / s)
            dtb = np.abs(tb) * ds / np.abs(s) + U * np.abs(tb) + TINY
            fin = np.isfinite(d).all(1) & (dd > 0)
            out["meets"] = fin & (disc >= 0) & (s / dd > 0)
            out["tb"] = np.where(out["meets"], tb, 0.0)
            out["yes"] = fin & (disc > KF * ddisc) & (s > KF * ds)
            out["no"] = ~fin | (disc < -KF * ddisc) | ((disc >= 0) & (s < -KF * ds)) | ((disc < 0) & (b < -KF * (db + np.sqrt(KF * ddisc))))
            out["tb_lo"] = np.where(cc <= 0, 0.0, tb - KF * dtb)                 # (cc is the rule's own float32 value: its cut is not in doubt)
            out["tb_hi"] = np.where(cc <= 0, 0.0, np.maximum(tb, 0.0) + KF * dtb)
    for k in ("tb_lo", "tb_hi"):
        out[k] = np.where(np.isfinite(out[k]), out[k], np.where(k == "tb_lo", -np.inf, np.inf))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------

class Case:
    """pos, nrm [Nt,3], shift [Nt,2] f32 of the whole grid; ids: the listed texels; bodies [Kbuf,16] f32, the first K of them are the call's; sets: M masks"""

    def __init__(self, name, geo, pos, nrm, shift, ids, N, mode, bodies, sets, K=None):
        self.name, self.geo = name, geo
        self.pos, self.nrm = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.Nt = self.pos.shape[0]
        self.shift = np.ascontiguousarray(shift, F32).reshape(self.Nt, 2)
        self.ids = np.ascontiguousarray(ids, np.int32)
        self.N, self.mode = int(N), mode
        self.buf = np.ascontiguousarray(bodies, F32).reshape(-1, 16)
        self.K = self.buf.shape[0] if K is None else int(K)
        self.bodies = self.buf[:self.K]
        self.sets = [int(s) & 0xFFFFFFFF for s in sets]
        self.M = len(self.sets)
        self.parts = TC.n_parts(self.N, "group")
        self._ref = None

    def masks(self):
        """the sets as the call takes them: what bits at or above K name is ignored"""
        return [s & ((1 << self.K) - 1) for s in self.sets]

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
        m_yes, m_no = np.zeros((Kb, R), bool), np.ones((Kb, R), bool)
        for k in range(Kb):
            B = body64(x32, d, bd / KF, c.bodies[k])
            m_yes[k], m_no[k] = B["yes"], B["no"]
            with np.errstate(invalid="ignore"):
                blocked[k] = B["yes"][:, None] & (B["tb_hi"][:, None] < t_lo)
                clear[k] = B["no"][:, None] | (B["tb_lo"][:, None] > t_hi)
                front64[k] = B["meets"][:, None] & (B["tb"][:, None] < t_s)
        cand_ok = ok[:, :C]
        self.overflow = int(rays.overflow.sum())

        def per_sample(x_, fn, init):
            out = np.full((P * N,) + x_.shape[1:], init, x_.dtype)
            fn.at(out, si, x_)
            return out.reshape((P, N) + x_.shape[1:])
        # the sets
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
        # counts per sample over every valid body, whatever the sets
        meet_yes = m_yes.any(0) if Kb else np.zeros(R, bool)
        meet_maybe = ~(m_no.all(0)) if Kb else np.zeros(R, bool)
        any_bl = blocked.any(0) if Kb else np.zeros((R, C), bool)
        all_cl = clear.all(0) if Kb else np.ones((R, C), bool)
        blk_yes = ~ok[:, C] & np.where(cand_ok, any_bl, True).all(1) & cand_ok.any(1)
        blk_maybe = (cand_ok & ~all_cl).any(1)
        unc_ray = (meet_maybe & ~meet_yes) | (meet_maybe & (cand_ok & ~any_bl & ~all_cl).any(1))
        self.meet_yes = per_sample(meet_yes, np.logical_and, True)               # [P, N]: every variant
        self.meet_maybe = per_sample(meet_maybe, np.logical_or, False)
        self.blk_yes = per_sample(blk_yes, np.logical_and, True)
        self.blk_maybe = per_sample(blk_maybe, np.logical_or, False)
        self.uncertain = per_sample(unc_ray, np.logical_or, False)
        self.scale = 2.0 * math.pi / N

    def caps(self):
        """(rays that overflow, share of the samples that may meet a body in which anything is uncertain)"""
        return self.overflow, float(self.uncertain.sum()) / max(int(self.meet_maybe.sum()), 1)

    def counts(self):
        """over the LIST (a duplicate counts again): (met lo, met hi, blocked lo, blocked hi)"""
        rows = np.array([self.row_of[int(t)] for t in self.case.ids], np.int64)
        g = lambda a: int(a[rows].sum())
        return g(self.meet_yes), g(self.meet_maybe), g(self.blk_yes), g(self.blk_maybe)

    def all_blocked(self, m):
        """[P] bool: every sample of the texel is, for set m, either certainly without an accepted hit or certainly blocked, and at least one is blocked --
        the texels on which lost[m] must equal irt_generate bit for bit"""
        irt = self.irt
        lo, hi = self.lo[m], self.hi[m]
        same = ((lo == irt.lo) & (hi == irt.hi)).all(2)                          # the sample's interval is the estimator's own: nothing of it can be clear
        sure = irt.n_out == 1                                                    # one admissible outcome: the hit (or the miss) is not in doubt
        return (same & sure).all(1) & (np.abs(self.mid[m]).sum((1, 2)) > 0)

    def summary(self):
        over, unc = self.caps()
        a, b, c_, d_ = self.counts()
        return {"texels": len(self.tex), "samples": int(self.meet_maybe.size), "may_meet": int(self.meet_maybe.sum()), "uncertain_share": unc, "overflow": over,
                "met": [a, b], "blocked": [c_, d_], "lost_share": [float((np.abs(m_).sum((1, 2)) > 0).mean()) for m_ in self.mid]}


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
        a, b, c_, d_ = ref.counts()
        s = [int(v) for v in np.asarray(stats).reshape(-1)[:2]]
        if not a <= s[0] <= b:
            fails.append("stats[0] = %d outside [%d, %d]" % (s[0], a, b))
        if not c_ <= s[1] <= d_:
            fails.append("stats[1] = %d outside [%d, %d]" % (s[1], c_, d_))
    print("error/bound irt_shadow %-40s %s" % (case.name + " " + what, "rejected" if fails else "%.4f" % worst))
    if fails:
        raise AssertionError("%s %s:\n%s" % (case.name, what, "\n".join(fails)))
    RATIOS[case.name] = max(RATIOS.get(case.name, 0.0), worst)
    return worst


# ---- float32 restatement of the rule (CPU), op by op, with the mutants the check must reject ------------------------------------------------------------------------

MUTANTS = ("one_sided", "shell", "naive_root", "no_compare", "add_missed", "sum_sets", "high_bits", "pi")


def quad_f32(rec, x, d, mut=None):
    """-> (meets [R] bool, t_b [R] f32): the header's sequence; x, d [R,3] f32"""
    o, m, mm, ua, vb = quad_record_f32(rec)
    with np.errstate(all="ignore"):
        if not (np.isfinite(mm) and mm > 0):
            return np.zeros(len(x), bool), np.zeros(len(x), F32)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        den = (m[0] * dx + m[1] * dy) + m[2] * dz
        q = [o[i] - x[:, i] for i in range(3)]
        num = (m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]
        t = (num / den).astype(F32)
        h = [t * d[:, i] - q[i] for i in range(3)]
        u = (h[0] * ua[0] + h[1] * ua[1]) + h[2] * ua[2]
        v = (h[0] * vb[0] + h[1] * vb[1]) + h[2] * vb[2]
        meets = (den != 0) & np.isfinite(t) & (t > 0) & (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
        if mut == "one_sided":
            meets &= den < 0                                                     # the emitting side only, as the lobe sample of speclight.hip asks
    return meets, np.where(meets, t, F32(0)).astype(F32)


def ball_f32(rec, x, d, mut=None):
    rec = np.asarray(rec, F32)
    c, r = rec[1:4], rec[4]
    with np.errstate(all="ignore"):
        rr = r * r
        oc = [c[i] - x[:, i] for i in range(3)]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        b = (oc[0] * dx + oc[1] * dy) + oc[2] * dz
        dd = (dx * dx + dy * dy) + dz * dz
        cc = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - rr
        disc = b * b - dd * cc
        sq = np.sqrt(np.maximum(disc, F32(0))).astype(F32)
        s = b + sq
        far = s / dd
        meets = (disc >= 0) & (far > 0)
        near = ((b - sq) / dd) if mut == "naive_root" else (cc / s)
        tb = np.where(cc <= 0, F32(0), near).astype(F32)
        if mut == "shell":
            meets &= cc > 0                                                      # the surface only: from inside nothing is entered
    return meets, np.where(meets, tb, F32(0)).astype(F32)


_TRACED = {}


def traced(case):
    """float32 brute-force hits of the case's samples, shared by every mutant: (L unique texels, dirs [P,N,3], t, pid, radiance [R,3])"""
    if case.name not in _TRACED:
        from oracle import oracle as O
        L = np.unique(case.ids.astype(np.int64))
        d = O.generate_dir(case.nrm[L], case.N, case.mode, case.shift[L])
        t, pid, uv = TC.trace_f32(case.geo, np.repeat(case.pos[L], case.N, 0), d.reshape(-1, 3))
        _TRACED[case.name] = (L, d, t, pid, TC.shade_f32(case.geo, t, pid, uv))
    return _TRACED[case.name]


def shadow_f32(case, mut=None, sentinel=SENTINEL):
    """-> (lost [M,Nt,3] f32, stats [2]); unlisted texels hold the sentinel"""
    c = case
    L, d, t, pid, rad = traced(c)
    P, N = len(L), c.N
    x, dr = np.repeat(c.pos[L], N, 0), d.reshape(-1, 3)
    accepted = np.isfinite(t) & (t > F32(1e-4)) & (pid >= 0)
    recs = c.buf if mut == "high_bits" else c.bodies
    Kb = len(recs)
    met, tb = np.zeros((Kb, P * N), bool), np.zeros((Kb, P * N), F32)
    for k in range(Kb):
        kind = LC.record_kind(recs[k])
        if kind == "quad":
            met[k], tb[k] = quad_f32(recs[k], x, dr, mut)
        elif kind == "sphere":
            met[k], tb[k] = ball_f32(recs[k], x, dr, mut)
    with np.errstate(invalid="ignore"):
        front = met & (np.ones_like(tb, bool) if mut == "no_compare" else (tb < t[None]))
    take = np.ones(P * N, bool) if mut == "add_missed" else accepted
    Lr = np.where(accepted[:, None], rad, F32(1)).astype(F32)                    # (add_missed: a ray that leaves the scene carries radiance 1)
    out = np.full((c.M, c.Nt, 3), sentinel, F32)
    for m, mask in enumerate(c.sets if mut == "high_bits" else c.masks()):
        ks = [k for k in range(Kb) if mask >> k & 1]
        if mut == "sum_sets":
            w = front[ks].sum(0).astype(F32) if ks else np.zeros(P * N, F32)
        else:
            w = (front[ks].any(0) if ks else np.zeros(P * N, bool)).astype(F32)
        terms = (Lr * (w * take)[:, None]).astype(F32)
        v = TC.estimator_f32(c.nrm[L], d, terms.reshape(P, N, 3), False, "group", c.parts)
        out[m, L] = v * F32(0.5) if mut == "pi" else v
    mult = np.bincount(np.searchsorted(L, c.ids.astype(np.int64)), minlength=P)
    anymet = met.any(0).reshape(P, N) if Kb else np.zeros((P, N), bool)
    anyfront = (front.any(0) & accepted).reshape(P, N) if Kb else np.zeros((P, N), bool)
    return out, np.array([(anymet * mult[:, None]).sum(), (anyfront * mult[:, None]).sum()], np.int64)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------------------------

def quad(o, a, b):
    """checked by the shipped helper: the valid records under test are the ones a user gets"""
    from texir_code_amd import irtlight
    return irtlight.quad(o, a, b)


def ball(c, r):
    from texir_code_amd import irtlight
    return irtlight.sphere(c, r)


_GEO = {}


def box_open():
    """the golden box without its ceiling (the two triangles whose corners all lie at y = 3): rays leave through the top"""
    if "open" not in _GEO:
        geo, _ = TC.golden_geo("box")
        keep = ~(geo.verts[geo.tris][:, :, 1] == geo.verts[:, 1].max()).all(1)
        assert keep.sum() == geo.T - 2
        uv = geo.tri_uvs.reshape(-1, 3, 2)[keep].reshape(-1, 2)
        _GEO["open"] = TC.Geo("box_open", geo.verts, geo.tris[keep], uv, geo.hdr)
    return _GEO["open"]


def box_const(L=1.5):
    """the golden box with a constant radiance texture"""
    if "const" not in _GEO:
        geo, _ = TC.golden_geo("box")
        _GEO["const"] = TC.Geo("box_const", geo.verts, geo.tris, geo.tri_uvs, np.full(geo.hdr.shape, L, F32))
    return _GEO["const"]


def spread(scene, n):
    """n valid texels spread over every face of the atlas"""
    _, gb = TC.golden_geo(scene)
    v = np.argwhere(gb["valid"].reshape(-1) > 0)[:, 0]
    return v[:: max(1, len(v) // n)][:n]


def with_inside(ids, rec, n):
    """the list with its last n entries replaced by valid texels INSIDE the ball `rec`"""
    _, gb = TC.golden_geo("box")
    p = gb["pos"].reshape(-1, 3).astype(F64)
    inside = np.argwhere((gb["valid"].reshape(-1) > 0) & (((p - rec[1:4].astype(F64)) ** 2).sum(1) < 0.81 * float(rec[4]) ** 2))[:, 0]
    inside = np.setdiff1d(inside, ids[:-n])[:n]
    assert len(inside) == n, len(inside)
    return np.concatenate([ids[:-n], inside])


def floor_ids(n=None):
    _, gb = TC.golden_geo("box")
    v = np.argwhere((gb["valid"].reshape(-1) > 0) & (gb["nrm"].reshape(-1, 3)[:, 1] > 0.9))[:, 0]
    return v if n is None else v[:n]


# the box is [0, 8] x [0, 3] x [0, 6]; texels sit 0.01 inside their faces
PANEL = lambda: quad([3.0, 2.5, 2.0], [2.0, 0.0, 0.0], [0.0, 0.0, 2.0])           # a x b = (0, -4, 0): it shines down; ceiling texels meet its back
BALL = lambda: ball([4.0, 1.25, 3.0], 0.5)
OUTSIDE = lambda: ball([-2.5, 1.5, 3.0], 1.0)                                      # behind the wall x = 0: met, never in front of the scene's hit
FAR = lambda: ball([40.0, 50.0, -30.0], 2.0)                                       # met by a few rays, far behind every wall


def eight_records():
    nan_rec = PANEL().copy()
    nan_rec[2] = np.nan
    bad_kind = BALL().copy()
    bad_kind[0] = 2.0
    return np.stack([
        ball([2.0, 1.0, 2.0], 0.75),                                               # 0 and 1 overlap: the sets {0}, {1}, {0, 1}
        ball([2.5, 1.25, 2.25], 0.75),
        nan_rec,                                                                   # a NaN word: never blocks
        quad([0.0, 1.5, 0.0], [8.0, 0.0, 0.0], [0.0, 0.0, 6.0]),                  # a horizontal sheet at half height, wall to wall: edge-on to wall texels' grazing rays
        bad_kind,                                                                  # an unknown kind: never blocks
        ball([7.99, 1.5, 3.0], 1.0),                                               # around wall texels of x = 8: they are INSIDE it, t_b = 0
        ball([6.0, 2.0, 5.0], 0.05),                                               # tiny: most passes meet it in no lane, some in one
        quad([5.0, 0.5, 1.0], [0.5, 1.0, 0.25], [-0.25, 0.5, 1.0]),               # tilted: every component of m
    ])


_CASES = {}


def case(name):
    if name in _CASES:
        return _CASES[name]
    geo, gb = TC.golden_geo("room" if name.startswith("room") else "box")
    pos, nrm, shift = gb["pos"].reshape(-1, 3), gb["nrm"].reshape(-1, 3), gb["shift"].reshape(-1, 2)
    if name == "box_three":                                                        # 130 texels (two waves and two lanes), 8 parts
        c = Case(name, geo, pos, nrm, shift, spread("box", 130), 64, "uniform", np.stack([PANEL(), BALL(), OUTSIDE()]), [1, 2, 4, 7, 3])
    elif name == "box_eight":                                                      # 65 texels, 32 parts, the cosine mode, every kind of record, every kind of mask
        c = Case(name, geo, pos, nrm, shift, with_inside(spread("box", 65), eight_records()[5], 6), 256, "cosine", eight_records(), [1, 2, 3, 0, 0xFFFFFF00 | 8, 0xFF, 0x20, 0x40 | 0x80])
    elif name == "box_eight_small":                                                # the same records at a size the CPU restatement and its mutants afford
        c = Case(name, geo, pos, nrm, shift, with_inside(spread("box", 40), eight_records()[5], 6), 64, "uniform", eight_records(), [1, 2, 3, 0, 0xFFFFFF00 | 8, 0xFF, 0x20, 0x40 | 0x80])
    elif name == "box_inside":                                                     # every texel inside one ball: every ray meets it at t_b = 0
        c = Case(name, geo, pos, nrm, shift, spread("box", 63), 3, "uniform", ball([4.0, 1.5, 3.0], 20.0)[None], [1])
    elif name == "box_inside256":                                                  # the same at 32 parts
        c = Case(name, geo, pos, nrm, shift, spread("box", 65), 256, "uniform", ball([4.0, 1.5, 3.0], 20.0)[None], [1])
    elif name == "box_one":                                                        # one texel, one sample, one body, two sets
        c = Case(name, geo, pos, nrm, shift, floor_ids()[80:81], 1, "uniform", ball([4.0, 1.5, 3.0], 20.0)[None], [1, 0])
    elif name == "box_nobody":                                                     # K = 0
        c = Case(name, geo, pos, nrm, shift, spread("box", 65), 64, "uniform", np.zeros((0, 16), F32), [1])
    elif name == "box_highbits":                                                   # K = 1 of a buffer of two: bit 1 names no body of the call
        c = Case(name, geo, pos, nrm, shift, spread("box", 63), 64, "uniform", np.stack([BALL(), PANEL()]), [1, 2, 3], K=1)
    elif name == "box_open_top":                                                   # a ball above the open top: met only by rays that leave the scene
        c = Case(name, box_open(), pos, nrm, shift, floor_ids(65), 64, "uniform", np.stack([ball([4.0, 6.0, 3.0], 1.5), BALL()]), [1, 2])
    elif name == "box_back":                                                       # ceiling texels only: the panel is met from its back
        _, gbb = TC.golden_geo("box")
        v = np.argwhere((gbb["valid"].reshape(-1) > 0) & (gbb["nrm"].reshape(-1, 3)[:, 1] < -0.9))[:, 0]
        c = Case(name, geo, pos, nrm, shift, v[:63], 64, "uniform", PANEL()[None], [1])
    elif name == "box_overlap":                                                    # two overlapping balls and the sets {0}, {1}, {0, 1}
        c = Case(name, geo, pos, nrm, shift, floor_ids(65), 64, "uniform", eight_records()[:2], [1, 2, 3])
    elif name == "box_cover":                                                      # a large quad 2^-10 above the floor texels: whatever they receive is blocked
        c = Case(name, geo, pos, nrm, shift, floor_ids(), 64, "uniform", np.stack([cover_quad(), FAR()]), [1, 2, 3])
    elif name == "box_tangent":                                                    # a ball of radius 2048 under the floor whose top rises 2^-11 above it, seen from the ceiling
        _, gbb = TC.golden_geo("box")
        v = np.argwhere((gbb["valid"].reshape(-1) > 0) & (gbb["nrm"].reshape(-1, 3)[:, 1] < -0.9))[:, 0]
        c = Case(name, geo, pos, nrm, shift, v[:130], 64, "uniform", ball([4.0, -2048.0 + 2.0 ** -11, 3.0], 2048.0)[None], [1])
    elif name == "box_below":                                                      # bodies under the floor: no ray of a floor texel meets them
        c = Case(name, geo, pos, nrm, shift, floor_ids(65), 64, "uniform",
                 np.stack([ball([4.0, -5.0, 3.0], 1.0), quad([0.0, -1.0, 0.0], [8.0, 0.0, 0.0], [0.0, 0.0, 6.0])]), [1, 2, 3])
    elif name == "room_two":
        c = Case(name, geo, pos, nrm, shift, spread("room", 130), 64, "uniform", np.stack([PANEL(), BALL()]), [1, 2])
    elif name == "room_small":
        c = Case(name, geo, pos, nrm, shift, spread("room", 10), 64, "uniform", np.stack([PANEL(), BALL()]), [1, 2, 3])
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def cover_quad():
    """2^-10 above the floor texels' height 0.01, far larger than the box: rays down to the smallest cos(theta) of N = 64 enter it before they reach a wall"""
    y = float(F32(0.01)) + 2.0 ** -10
    return quad([-4096.0, y, -4096.0], [0.0, 0.0, 8192.0], [8192.0, 0.0, 0.0])    # a x b = (0, -1, 0) * 2^26: it shines down


GPU_CASES = ("box_three", "box_eight", "box_eight_small", "box_inside", "box_inside256", "box_one", "box_nobody", "box_highbits", "box_open_top", "box_back", "box_overlap",
             "box_cover", "box_below", "box_tangent", "room_two", "room_small")
CPU_CASES = ("box_three", "box_eight_small", "box_inside", "box_inside256", "box_one", "box_nobody", "box_highbits", "box_open_top", "box_back", "box_overlap", "box_cover",
             "box_below", "box_tangent", "room_small")
# where each mutant must be rejected
MUTANT_CASES = {"one_sided": "box_back", "shell": "box_eight_small", "naive_root": "box_tangent", "no_compare": "box_three", "add_missed": "box_open_top",
                "sum_sets": "box_overlap", "high_bits": "box_highbits", "pi": "box_three"}


# ---- the analytic pin of the reference ------------------------------------------------------------------------------------------------------------------------------------

def pin_case(N=4096, alpha=0.3, beta=0.6, L=1.5):
    """one floor point of the constant-radiance box under a ball of angular radius alpha whose centre makes the angle beta with the normal"""
    geo = box_const(L)
    x = np.array([[4.0, 0.01, 3.0]], F32)
    n = np.array([[0.0, 1.0, 0.0]], F32)
    dist = 1.25
    ctr = x[0].astype(F64) + dist * np.array([math.sin(beta), math.cos(beta), 0.0])
    rec = ball(ctr, dist * math.sin(alpha))
    sh = np.array([[0.37, 0.61]], F32)
    return Case("pin", geo, x, n, sh, [0], N, "uniform", rec[None], [1]), math.pi * L * math.sin(alpha) ** 2 * math.cos(beta), L
