"""Float64 restatement of the GGX importance-sampled specular chain (generate_dir, utils/sample_util.py:63-146; render + specular_reflectance,
models/mat_nvdiffrast.py:201-279) PER SAMPLE, the rounding-error bound its comparisons use, the kink variants, check functions, seeded case
generators and operator mutants.  Shared by test_spec_ref_cpu.py (no GPU) and test_gpu_spec_kernels.py (no tests here).

The restatement works on float32 inputs held in float64 and never rounds.  The only float32 roundings it has are the ones that are part of the
reference's DEFINITION: the Hammersley points, the clamp edges float32(1e-6), float32(1 - 1e-6), float32(0.99), float32(1e-4), float32(clamp_eps).

THE BOUND (running error analysis by autograd).  The result of every elementary float32 operation of the chain -- each add, multiply, divide, sqrt, sin,
cos, exp2, each product and partial sum of a dot product, every constant that float32 has to round -- passes through Tape.__call__:
x -> x * (1 + e_j), e_j a zero tensor with one entry per sample.  For a per-sample output y

    bound(y) = K * sum_j |dy / de_j| * (u + 2^-126 / |x_j|)           u = 2^-24, K = 4 (both from texture_cases)

is what float32 rounding (and one flushed denormal per operation) can do to y to first order; one autograd pass gives it for all samples.  d w / d r is
carried by dual numbers (class D) whose every tangent operation goes through the same hook, so bound(dw) is the same formula.  Exact operations
(times 2, 4, 1/8, selections, negation, products with the 0 / 1 axis) have no hook.

KINKS.  Every branch of the chain is a Kink (name, quantity q, edge c, side).  q of a sample is UNCERTAIN when |q - c| <= bound(q) and bound(q) > 0.
A sample with k <= 4 uncertain kinks is evaluated in all 2^k branch combinations (variants); one with more is left out (cap: 0.1 % of a case).
  value (w, l, directions): continuous across a clamp -> compared with the variant whose clamp branches are the natural ones, inside the MAXIMUM of the
        bounds of the variants that differ from it in clamp branches only; a wrap or the axis choice is not continuous -> ONE such group must accept;
  derivative (dw): within the bound of ONE variant;
  per-pixel sum: inside the sum of its samples' intervals [min over variants - bound, max over variants + bound] plus the accumulation term.
"""
import math
import os

import numpy as np
import torch

from oracle import mat_step as MS
from texture_cases import K, TINY, U

F32 = np.float32
HI = float(F32(1.0 - 1e-6))
LO = float(F32(1e-6))
AXIS_EDGE = float(F32(0.99))
LV_EPS = float(F32(1e-4))
MAX_UNC = 4
CAP_LEFT_OUT = 1e-3          # share of samples with more than MAX_UNC uncertain kinks
CAP_MULTI_SMOOTH = 0.03      # share of multi-variant samples in the smooth families
CAP_NONBASE = 0.02           # share of samples accepted by a variant other than the base one (random-input families)
DISC = ("axis", "wrap0_hi", "wrap0_lo", "wrap1_hi", "wrap1_lo")

MUTANTS = ("k_r2_half", "fresnel_swapped", "axis_09", "dots_unit_normal", "no_4vdh_over_ndh", "cos_sign", "wrap_ge", "clamp_grad_outside",
           "ct_den_term_dropped", "dalbedo_no_pi", "inv_S_is_64", "ceps_ignored")


def lanes_per_pixel(S, forced=0):
    """documented lane assignment of the specular kernels: S lanes when S is a power of two <= 64, else 64; TEXIR_SPEC_LPP forces fewer"""
    lpp = S if (S <= 64 and S & (S - 1) == 0) else 64
    return forced if 1 <= forced <= lpp else lpp


def n_acc(S, forced_lpp=0):
    """roundings one term of a per-pixel sum passes through: the product with the lighting (1), one add per pass and one per shuffle level, the
    division by S (1)"""
    lpp = lanes_per_pixel(S, forced_lpp)
    return 1 + (S + lpp - 1) // lpp + int(math.log2(lpp)) + 1


# ---- hooks and dual numbers --------------------------------------------------------------------------------------------------------------------

class Tape:
    def __init__(self, on=True):
        self.on, self.es, self.wt = on, [], []

    def __call__(self, x):
        if not self.on:
            return x
        e = torch.zeros_like(x, requires_grad=True)
        self.es.append(e)
        self.wt.append(K * (U + TINY / torch.clamp(x.detach().abs(), min=TINY)))
        return x * (1 + e)

    def bound(self, y):
        """[M,1] -> [M,1]"""
        if not (self.on and y.requires_grad):
            return torch.zeros_like(y.detach())
        gs = torch.autograd.grad(y.sum(), self.es, retain_graph=True, allow_unused=True)
        out = torch.zeros_like(y.detach())
        for g, w in zip(gs, self.wt):
            if g is not None:
                out += (g.abs() * w).sum(-1, keepdim=True)
        return out


class D:
    """value and tangent (None = identically zero)"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v, self.d = v, d


class Kink:
    def __init__(self, q, edge, op, nat):
        self.q, self.edge, self.op, self.nat = q, edge, op, nat


class Chain:
    """the sample chain on flat per-sample tensors [M,k].  tape off + dtype float32 = the chain in float32 op by op.  dual=False: r is an autograd
    leaf instead (reverse mode on the plain expression)."""

    def __init__(self, inp, ceps, tape, force=None, mut=None, dual=True, mode="importance"):
        self.i, self.R, self.force, self.mut, self.dual, self.mode = inp, tape, force or {}, mut, dual, mode
        self.dtype = inp["n"].dtype
        self.ceps = float(F32(1e-30 if mut == "ceps_ignored" else ceps))
        self.kinks = {}
        self.M = inp["n"].shape[0]

    def C(self, c):
        """a constant float32 has to round"""
        return self.R(torch.full((self.M, 1), c, dtype=self.dtype))

    # dual arithmetic: every value and every tangent result is hooked
    def mul(self, a, b):
        R = self.R
        v = R(a.v * b.v)
        if a.d is None and b.d is None:
            return D(v)
        if a.d is None:
            return D(v, R(a.v * b.d))
        if b.d is None:
            return D(v, R(a.d * b.v))
        return D(v, R(R(a.d * b.v) + R(a.v * b.d)))

    def add(self, a, b, sign=1.0):
        R = self.R
        v = R(a.v + sign * b.v)
        if a.d is None and b.d is None:
            return D(v)
        if a.d is None:
            return D(v, sign * b.d)
        if b.d is None:
            return D(v, a.d)
        return D(v, R(a.d + sign * b.d))

    def sub(self, a, b):
        return self.add(a, b, -1.0)

    def div(self, a, b):
        R = self.R
        q = R(a.v / b.v)
        if a.d is None and b.d is None:
            return D(q)
        if b.d is None:
            return D(q, R(a.d / b.v))
        num = -R(q * b.d) if a.d is None else R(a.d - R(q * b.d))
        return D(q, R(num / b.v))

    def sqrt(self, a):
        R = self.R
        pos = a.v > 0
        s = R(torch.where(pos, torch.sqrt(torch.where(pos, a.v, torch.ones_like(a.v))), torch.zeros_like(a.v)))
        return D(s, None if a.d is None else R(a.d / (2 * s)))

    @staticmethod
    def times(a, c):
        """exact scaling by a power of two or a sign"""
        return D(a.v * c, None if a.d is None else a.d * c)

    def dot(self, a, b):
        m = [self.mul(a[k], b[k]) for k in range(3)]
        return self.add(self.add(m[0], m[1]), m[2])

    def unit(self, x):
        ln = self.add(self.sqrt(self.dot(x, x)), D(self.C(1e-6)))
        return [self.div(x[k], ln) for k in range(3)]

    # branches
    def kink(self, name, q, edge, op):
        nat = (q > edge) if op == "gt" else (q >= edge) if op == "ge" else (q < edge)
        self.kinks[name] = Kink(q, edge, op, nat.detach())
        if name in self.force:
            mask, side = self.force[name]
            return torch.where(mask, side, nat)
        return nat

    def clamp(self, a, name, lo=None, hi=None):
        v, d = a.v, a.d
        out = torch.zeros_like(v, dtype=torch.bool)
        if lo is not None:
            s = self.kink(name + "_lo", a.v, lo, "lt")
            v, out = torch.where(s, torch.full_like(v, lo), v), out | s
        if hi is not None:
            s = self.kink(name + "_hi", a.v, hi, "gt")
            v, out = torch.where(s, torch.full_like(v, hi), v), out | s
        if d is not None and self.mut != "clamp_grad_outside":
            d = torch.where(out, torch.zeros_like(d), d)         # torch.clamp: the gradient passes on the closed interval
        return D(v, d)

    def frame(self):
        i = self.i
        n = [D(i["n"][:, k:k + 1]) for k in range(3)]
        side = self.kink("axis", n[0].v.abs(), float(F32(0.9)) if self.mut == "axis_09" else AXIS_EDGE, "gt")
        nn = self.unit(n)
        z = torch.zeros_like(nn[0].v)
        # cross(axis, n) with axis = e_y (side) or e_x: products with 0 and 1 are exact
        c = [D(torch.where(side, nn[2].v, z)), D(torch.where(side, z, -nn[2].v)), D(torch.where(side, -nn[0].v, nn[1].v))]
        Uv = self.unit(c)
        Vv = self.unit(self.cross(nn, Uv))
        return n, nn, Uv, Vv

    def cross(self, a, b):
        c = lambda p, q: self.sub(self.mul(a[p], b[q]), self.mul(a[q], b[p]))
        return [c(1, 2), c(2, 0), c(0, 1)]

    def shifted(self, k):
        R = self.R
        one = 1.0
        s = self.i["ham"][:, k:k + 1] + self.i["sh"][:, k:k + 1]
        if self.dtype == torch.float64:
            # both terms are float32 inputs: where their sum is a float32 number, float32 computes it exactly -- no rounding, and the sample lies on the
            # side of the wrap the reference says (a sum of exactly 1 is NOT wrapped)
            s = torch.where(s.float().double() == s, s, R(s))
        side = self.kink("wrap%d_hi" % k, s, one, "ge" if self.mut == "wrap_ge" else "gt")
        s = torch.where(side, R(s - one), s)
        side = self.kink("wrap%d_lo" % k, s, 0.0, "lt")
        s = torch.where(side, R(s + one), s)
        return self.clamp(D(s), "s%d" % k, LO, HI).v

    def polar(self, s0):
        one = D(torch.ones_like(s0))
        if self.mode == "uniform":
            ct = D(self.R(1.0 - s0))
            return ct, self.sqrt(self.sub(one, self.mul(ct, ct)))
        if self.mode == "cosine":
            ct = self.sqrt(D(self.R(1.0 - s0)))
            return ct, self.sqrt(self.sub(one, self.mul(ct, ct)))
        rr = self.rr
        a = self.mul(rr, rr)
        den = self.add(one, self.mul(self.sub(self.mul(a, a), one), D(s0)))
        if self.mut == "ct_den_term_dropped":
            den = D(den.v)
        ct = self.sqrt(self.div(D(self.R(1.0 - s0)), den))
        ct = self.clamp(ct, "ct", None, HI)          # ct >= 0: the lower edge -(1 - 1e-6) cannot be reached
        st = self.sqrt(self.sub(one, self.mul(ct, ct)))
        st = self.clamp(st, "st", None, HI)
        return ct, st

    def direction(self):
        R = self.R
        n, nn, Uv, Vv = self.frame()
        s0, s1 = self.shifted(0), self.shifted(1)
        if self.mode == "importance":
            r = self.i["r"]
            self.rr = D(r, torch.ones_like(r)) if self.dual else D(r)
        ct, st = self.polar(s0)
        phi = R(R(self.C(2 * math.pi) * s1) - self.C(math.pi))
        sp = self.mul(st, D(R(torch.sin(phi))))
        cp = self.mul(st, D(R(torch.cos(phi))))
        if self.mut != "cos_sign":
            cp = self.times(cp, -1.0)
        h = [self.add(self.add(self.mul(Vv[k], sp), self.mul(nn[k], ct)), self.mul(Uv[k], cp)) for k in range(3)]
        return n, nn, h

    def spec(self):
        """-> w (D), l (3 D)"""
        R, C = self.R, self.C
        n, nn, h = self.direction()
        rr = self.rr
        one = D(torch.ones_like(rr.v))
        v = [D(R(self.i["cam"][:, k:k + 1] - self.i["pts"][:, k:k + 1])) for k in range(3)]
        lv = self.sqrt(self.dot(v, v))
        s = self.kink("lv_lo", lv.v, LV_EPS, "lt")
        lv = D(torch.where(s, torch.full_like(lv.v, LV_EPS), lv.v))
        v = [self.div(v[k], lv) for k in range(3)]
        nd = nn if self.mut == "dots_unit_normal" else n
        vdh = self.clamp(self.dot(h, v), "vdh", 0.0, 1.0)
        l = [self.sub(self.mul(self.times(vdh, 2.0), h[k]), v[k]) for k in range(3)]
        ndl = self.clamp(self.dot(nd, l), "ndl", 0.0, 1.0)
        ndh = self.clamp(self.dot(nd, h), "ndh", 0.0, 1.0)
        ndv = self.clamp(self.dot(nd, v), "ndv", 0.0, 1.0)
        c1, c2 = (-6.98316, 5.55472) if self.mut == "fresnel_swapped" else (-5.55472, 6.98316)
        e = self.mul(self.sub(self.mul(D(C(c1)), vdh), D(C(c2))), vdh)
        p2 = R(torch.exp2(e.v))
        fr = self.add(D(C(0.04)), self.mul(D(C(0.96)), D(p2, None if e.d is None else R(R(p2 * C(math.log(2.0))) * e.d))))
        if self.mut == "k_r2_half":
            kk = self.times(self.mul(rr, rr), 0.5)
        else:
            r1 = self.add(rr, one)
            kk = self.times(self.mul(r1, r1), 0.125)
        omk = self.sub(one, kk)
        ce = self.ceps
        g1l = self.div(ndl, self.clamp(self.add(self.mul(ndl, omk), kk), "den_l", ce))
        g1v = self.div(ndv, self.clamp(self.add(self.mul(ndv, omk), kk), "den_v", ce))
        g = self.mul(g1l, g1v)
        brdf = self.div(self.mul(fr, g), self.clamp(self.mul(self.times(ndl, 4.0), ndv), "den_b", ce))
        if self.mut == "no_4vdh_over_ndh":
            w = self.mul(brdf, ndl)
        else:
            w = self.div(self.mul(self.times(self.mul(brdf, ndl), 4.0), vdh), self.clamp(ndh, "den_w", ce))
        return w, l


# ---- inputs per sample -------------------------------------------------------------------------------------------------------------------------

def sample_inputs(normal, rough, points, cam, shift, S, dtype=torch.float64):
    P = len(normal)
    rep = lambda x, k: torch.from_numpy(np.repeat(np.asarray(x, np.float32).reshape(P, k), S, 0)).to(dtype)
    ham = torch.from_numpy(np.tile(MS.hammersley_points(S), (P, 1))).to(dtype)
    inp = {"n": rep(normal, 3), "sh": rep(shift, 2), "ham": ham}
    if rough is not None:
        inp["r"] = rep(rough, 1)
    if points is not None:
        inp["pts"] = rep(points, 3)
        inp["cam"] = torch.from_numpy(np.asarray(cam, np.float32).reshape(1, 3)).to(dtype).expand(P * S, 3).contiguous()
    return inp


def _take(inp, idx):
    return {k: v[idx] for k, v in inp.items()}


# ---- the reference with its variants -------------------------------------------------------------------------------------------------------------

class Ref:
    """per-sample reference of one case: arrays [V,M] over the variants (variant 0 = every branch as the reference takes it)"""

    def __init__(self, M, names, V):
        z = lambda: np.full((V, M), np.nan)
        self.M, self.V, self.names = M, V, names
        self.val = {k: z() for k in names}
        self.bnd = {k: z() for k in names}
        self.adm = np.zeros((V, M), bool)
        self.unc = {}
        self.nunc = np.zeros(M, np.int64)
        self.dmask = np.zeros(M, np.int64)
        self.left = np.zeros(M, bool)

    @property
    def multi(self):
        return (self.nunc > 0) & ~self.left


def _eval(inp, ceps, mode, names, force):
    tape = Tape()
    ch = Chain(inp, ceps, tape, force=force, mode=mode)
    if mode == "spec":
        ch.mode = "importance"
        w, l = ch.spec()
        outs = {"w": w.v, "dw": w.d, "l0": l[0].v, "l1": l[1].v, "l2": l[2].v}
    else:
        _, _, h = ch.direction()
        outs = {"d0": h[0].v, "d1": h[1].v, "d2": h[2].v}
    vals = {k: outs[k].detach().numpy()[:, 0] for k in names}
    bnds = {k: tape.bound(outs[k]).numpy()[:, 0] for k in names}
    return ch, tape, vals, bnds


def reference(inp, ceps=1e-14, mode="spec", names=("w", "dw"), chunk=150000):
    """inp: sample_inputs(...).  mode 'spec' | 'uniform' | 'cosine' | 'importance' (directions only)"""
    M = inp["n"].shape[0]
    ref = Ref(M, names, 1 << MAX_UNC)
    # (the suite's conftest raises the process-wide OpenMP thread count to every core of the machine for the C oracle; torch shares that setting, and its
    # many small operations crawl when a job is granted fewer cores than the machine has: keep to what OMP_NUM_THREADS grants while the chain is evaluated)
    keep = torch.get_num_threads()
    torch.set_num_threads(min(keep, int(os.environ.get("OMP_NUM_THREADS") or 0) or keep))
    try:
        for a in range(0, M, chunk):
            _reference_chunk(ref, _take(inp, slice(a, min(M, a + chunk))), a, ceps, mode, names)
    finally:
        torch.set_num_threads(keep)
    return ref


def _reference_chunk(ref, inp, off, ceps, mode, names):
    m = inp["n"].shape[0]
    sl = slice(off, off + m)
    ch, tape, vals, bnds = _eval(inp, ceps, mode, names, None)
    unc, nat, rank = {}, {}, {}
    nunc = np.zeros(m, np.int64)
    dmask = np.zeros(m, np.int64)
    bq = {}                                         # the two edges of a clamp share their quantity: one pass
    for name, k in ch.kinks.items():
        b = bq[id(k.q)] if id(k.q) in bq else bq.setdefault(id(k.q), tape.bound(k.q))
        u = (((k.q.detach() - k.edge).abs() <= b) & (b > 0)).numpy()[:, 0]
        unc[name], nat[name], rank[name] = u, k.nat.numpy()[:, 0], nunc.copy()
        if name in DISC:
            dmask |= np.where(u, 1 << np.minimum(nunc, 62), 0)
        nunc += u
        ref.unc.setdefault(name, np.zeros(ref.M, bool))[sl] = u
    left = nunc > MAX_UNC
    ref.nunc[sl], ref.left[sl], ref.dmask[sl] = nunc, left, np.where(left, 0, dmask)
    for k in names:
        ref.val[k][0, sl], ref.bnd[k][0, sl] = vals[k], bnds[k]
    ref.adm[0, sl] = ~left
    del ch, tape
    nv = np.where(left, 1, 1 << np.minimum(nunc, MAX_UNC))
    for c in range(1, ref.V):
        idx = np.nonzero(nv > c)[0]
        if idx.size == 0:
            break
        force = {}
        for name in unc:
            u = unc[name][idx]
            if u.any():
                flip = u & (((c >> rank[name][idx]) & 1) == 1)
                force[name] = (torch.from_numpy(u)[:, None], torch.from_numpy(nat[name][idx] ^ flip)[:, None])
        _, _, vals, bnds = _eval(_take(inp, torch.from_numpy(idx)), ceps, mode, names, force)
        ok = np.ones(idx.size, bool)
        for k in names:
            ref.val[k][c, off + idx], ref.bnd[k][c, off + idx] = vals[k], bnds[k]
            ok &= np.isfinite(vals[k]) & np.isfinite(bnds[k])
        ref.adm[c, off + idx] = ok                # a forced branch on which the reference itself is not finite is not a variant


# ---- checks ----------------------------------------------------------------------------------------------------------------------------------------

RATIOS = {}
SHARES = {}


def _record(family, what, worst, ref, nonbase, skip):
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    s = SHARES.setdefault(family, {"multi": 0.0, "left": 0.0, "nonbase": 0.0})
    live = ~skip
    n = max(1, int(live.sum()))
    s["multi"] = max(s["multi"], float(ref.multi.mean()))
    s["left"] = max(s["left"], float(ref.left.mean()))
    s["nonbase"] = max(s["nonbase"], float((nonbase & live).sum()) / n)
    print("error/bound %-12s %-52s %.4f   multi %.4f left %.5f nonbase %.5f" % (family, what, worst, ref.multi.mean(), ref.left.mean(), (nonbase & live).sum() / n))


def _fail(family, what, ratio, got, ref, key):
    i = int(np.nanargmax(np.where(np.isfinite(ratio), ratio, np.inf)))
    raise AssertionError("%s %s: %d of %d samples outside the bound; worst at sample %d: got %r, reference %r, bound %.3e (error / bound %.3g), %d variants"
                         % (family, what, int((~(ratio <= 1)).sum()), ratio.size, i, float(got[i]), float(ref.val[key][0, i]), float(ref.bnd[key][0, i]),
                            float(ratio[i]), int(ref.adm[:, i].sum())))


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def check_value(got, ref, key, family, what="", extra=0.0, named=None, cap=None):
    """a per-sample VALUE (flat [M]); extra: additional absolute bound per sample (observation roundings)"""
    got = np.asarray(got, np.float64).reshape(-1)
    assert got.shape == (ref.M,)
    skip = ref.left
    assert np.isfinite(got[~skip]).all(), "%s %s: non-finite values" % (family, what)
    val, bnd = ref.val[key], ref.bnd[key] + extra
    V = ref.V
    maxb = np.zeros((V, ref.M))
    for c in range(V):
        gi = (c & ref.dmask)[None]
        cur = np.take_along_axis(maxb, gi, 0)
        np.put_along_axis(maxb, gi, np.where(ref.adm[c], np.maximum(cur[0], bnd[c]), cur[0])[None], 0)
    best = np.full(ref.M, np.inf)
    for g in range(V):
        isbase = ref.adm[g] & ((g & ~ref.dmask) == 0)
        best = np.where(isbase, np.minimum(best, _ratio(np.abs(got - val[g]), maxb[g])), best)
    base = _ratio(np.abs(got - val[0]), bnd[0])
    return _finish(best, base, got, ref, key, family, what, skip, named, cap)


def check_deriv(got, ref, key, family, what="", extra=0.0, named=None, cap=None):
    """a per-sample DERIVATIVE: inside the bound of ONE admissible variant"""
    got = np.asarray(got, np.float64).reshape(-1)
    assert got.shape == (ref.M,)
    skip = ref.left
    assert np.isfinite(got[~skip]).all(), "%s %s: non-finite values" % (family, what)
    best = np.full(ref.M, np.inf)
    for c in range(ref.V):
        best = np.where(ref.adm[c], np.minimum(best, _ratio(np.abs(got - ref.val[key][c]), ref.bnd[key][c] + extra)), best)
    base = _ratio(np.abs(got - ref.val[key][0]), ref.bnd[key][0] + extra)
    return _finish(best, base, got, ref, key, family, what, skip, named, cap)


def _finish(best, base, got, ref, key, family, what, skip, named, cap):
    best = np.where(skip, 0.0, best)
    worst = float(best.max()) if best.size else 0.0
    nonbase = ~(base <= 1) & (best <= 1) & ~skip
    if named is not None:                         # a case built ON a kink: count the samples that are not uncertain at it
        on = np.zeros(ref.M, bool)
        for nm in named:
            on |= ref.unc[nm]
        nonbase &= ~on
    _record(family, what, worst, ref, nonbase, skip)
    if not worst <= 1.0:
        _fail(family, what, best, got, ref, key)
    if cap is not None:
        n = max(1, int((~skip).sum()))               # (a share resolves 1 / n: one sample is always within the cap)
        assert nonbase.sum() <= max(1.0, cap * n), "%s %s: %d of %d samples only pass on a variant other than the base one (cap %.4f)" % (family, what, nonbase.sum(), n, cap)
    return worst


def intervals(ref, key):
    """per sample [min over variants - bound, max over variants + bound]"""
    lo = np.where(ref.adm, ref.val[key] - ref.bnd[key], np.inf).min(0)
    hi = np.where(ref.adm, ref.val[key] + ref.bnd[key], -np.inf).max(0)
    return lo, hi


def check_sum(got, coef, ref, key, const, const_abs, nr, family, what="", extra=0.0):
    """per-pixel sums got[P,C] = const[P,C] + sum_i coef[P,S,C] * x_i against the samples' intervals.  The accumulation adds
    K * u * (nr * sum_i |coef_i x_i| + 3 * |const| + |total|) (+ one flushed denormal per rounding) + extra; a pixel with a left-out sample is not
    compared."""
    got = np.asarray(got, np.float64)
    P, S, Cn = coef.shape
    assert got.shape == (P, Cn)
    lo, hi = intervals(ref, key)
    lo, hi = lo.reshape(P, S, 1), hi.reshape(P, S, 1)
    a, b = coef * lo, coef * hi
    with np.errstate(invalid="ignore"):
        LOs, HIs = np.minimum(a, b).sum(1) + const, np.maximum(a, b).sum(1) + const
        mag = np.maximum(np.abs(a), np.abs(b)).sum(1)
    acc = K * (U * (nr * mag + 3 * const_abs + np.maximum(np.abs(LOs), np.abs(HIs))) + (nr + 4) * TINY) + extra
    skip = ref.left.reshape(P, S).any(1)
    live = ~skip
    assert np.isfinite(got[live]).all(), "%s %s: non-finite values" % (family, what)
    mid, half = 0.5 * (LOs + HIs), 0.5 * (HIs - LOs) + acc
    ratio = np.where(skip[:, None], 0.0, _ratio(np.abs(got - mid), half))
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    print("error/bound %-12s %-52s %.4f   (pixels not compared: %d)" % (family, what, worst, int(skip.sum())))
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf))), ratio.shape)
        raise AssertionError("%s %s: %d of %d elements outside; worst at %s: got %r, interval [%r, %r] +- %.3e (ratio %.3g)"
                             % (family, what, int((~(ratio <= 1)).sum()), ratio.size, i, float(got[i]), float(LOs[i]), float(HIs[i]), float(acc[i]), worst))
    return worst


def check_exact(got, ref, bound, family, what=""):
    """plain element-wise comparison (d_albedo): |got - ref| <= bound"""
    from texture_cases import check
    worst = check(got, ref, bound, family, what)
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    return worst


def rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------

class Case:
    """one set of inputs of the specular kernels (float32 numpy), its lighting and incoming gradient, and the lazily built reference"""

    def __init__(self, name, family, normal, rough, points, cam, shift, S, seed, ceps=1e-14, light="random", grad="random", named=None, smooth=False):
        f = lambda x, k: np.ascontiguousarray(np.asarray(x, F32).reshape(-1, k))
        self.name, self.family, self.S, self.ceps, self.named, self.smooth = name, family, int(S), float(ceps), named, smooth
        self.normal, self.rough, self.points, self.shift = f(normal, 3), f(rough, 1)[:, 0].copy(), f(points, 3), f(shift, 2)
        self.cam = np.asarray(cam, F32).reshape(3)
        self.P = P = self.normal.shape[0]
        rng = np.random.default_rng([seed, P, self.S, 7])
        self.albedo = rng.random((P, 3), F32)
        self.irr = rng.random((P, 3), F32) * F32(2.0)
        self.L = make_light(light, P, self.S, rng)
        self.d_rgb = make_grad(grad, P, rng)
        self._ref = None

    def inputs(self, dtype=torch.float64):
        return sample_inputs(self.normal, self.rough, self.points, self.cam, self.shift, self.S, dtype)

    def ref(self):
        if self._ref is None:
            self._ref = reference(self.inputs(), self.ceps, "spec", ("w", "dw"))
        return self._ref

    # the per-pixel stage in float64
    def coef_rgb(self):
        return self.L.astype(np.float64) / self.S

    def coef_drough(self):
        return (self.L.astype(np.float64) * self.d_rgb.astype(np.float64)[:, None, :]).sum(-1, keepdims=True) / self.S

    def diffuse(self):
        return self.irr.astype(np.float64) * self.albedo.astype(np.float64) / math.pi

    def d_albedo(self):
        """(value, bound): two roundings and the float32 pi"""
        v = self.d_rgb.astype(np.float64) * self.irr.astype(np.float64) / math.pi
        return v, K * (3 * U * np.abs(v) + 3 * TINY)

    def check_rgb(self, got, family, what="", forced_lpp=0):
        return check_sum(got, self.coef_rgb(), self.ref(), "w", self.diffuse(), np.abs(self.diffuse()), n_acc(self.S, forced_lpp), family, what)

    def check_drough(self, got, family, what="", forced_lpp=0, ref=None, key="dw"):
        c = self.coef_drough()
        r = self.ref() if ref is None else ref
        # the dot product L . d_rgb in float32: 3 roundings carried by the sum of its absolute terms, times the largest |dw| of the sample's interval
        ca = (np.abs(self.L.astype(np.float64)) * np.abs(self.d_rgb.astype(np.float64))[:, None, :]).sum(-1, keepdims=True) / self.S
        lo, hi = intervals(r, key)
        m = np.maximum(np.abs(lo), np.abs(hi)).reshape(self.P, self.S, 1)
        with np.errstate(invalid="ignore"):
            dot_err = K * 3 * U * (ca * m).sum(1)
        dot_err = np.where(np.isfinite(dot_err), dot_err, 0.0)             # (a left-out sample: its pixel is not compared)
        got = np.asarray(got, np.float64).reshape(self.P, 1)
        z = np.zeros((self.P, 1))
        return check_sum(got, c, r, key, z, z, n_acc(self.S, forced_lpp), family, what, extra=dot_err)


def exact_ref(x):
    """a Ref of ONE variant with zero bound around given per-sample values (texir_spec_backward_ws is fed the float32-rounded dw: its inputs are exact)"""
    x = np.asarray(x, np.float64).reshape(-1)
    r = Ref(x.size, ("dw",), 1)
    r.val["dw"][0], r.bnd["dw"][0], r.adm[0] = x, 0.0, True
    return r


def make_light(kind, P, S, rng):
    if kind == "zeros":
        return np.zeros((P, S, 3), F32)
    if kind == "onehot":
        L = np.zeros((P, S, 3), F32)
        L[np.arange(P), rng.integers(0, S, P)] = 1.0
        return L
    if kind == "lamp":
        L = np.ones((P, S, 3), F32)
        L[np.arange(P), rng.integers(0, S, P)] = 1e4
        return L
    return np.exp(rng.normal(size=(P, S, 3))).astype(F32)


def make_grad(kind, P, rng):
    if kind == "zeros":
        return np.zeros((P, 3), F32)
    g = rng.normal(size=(P, 3)).astype(F32)
    if kind == "channel":
        g[:, 0] = 0
        g[:, 2] = 0
    return g


def unit_normals(P, rng):
    n = rng.normal(size=(P, 3))
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)


CAM = np.array([0.3, 1.5, -0.2], F32)


def front_points(n, rng, dist=(0.5, 3.0)):
    """points the camera sees from the front: camera - (direction in the normal's hemisphere) * distance"""
    P = len(n)
    d = rng.normal(size=(P, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    d = np.where(((d * n).sum(-1, keepdims=True) < 0), -d, d) + 0.3 * n
    return (CAM[None] - d * rng.uniform(*dist, (P, 1))).astype(F32)


def smooth_case(P, S, seed=0, rlo=0.05, rhi=0.8, name=None, family="A", **kw):
    rng = np.random.default_rng([seed, P, S])
    n = unit_normals(P, rng)
    r = rng.uniform(rlo, rhi, P).astype(F32)
    kw.setdefault("smooth", family == "A")
    return Case(name or "A_P%d_S%d" % (P, S), family, n, r, front_points(n, rng), CAM, rng.random((P, 2), F32), S, seed, **kw)


S_LIST = (1, 2, 4, 8, 16, 32, 64, 3, 24, 63, 65, 100, 128, 256, 1000)


def p_list(S):
    ppw = 64 // lanes_per_pixel(S)
    return sorted({p for p in (1, ppw - 1, ppw, ppw + 1, 4 * ppw + 1, 1037) if p >= 1})


SPECIAL_NORMALS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0.995, 0.0998, 0.0], [0.989, 0.1, 0.1], [0.75, 1.25, -0.5],
                            [0, 0, 0], [-0.3, 0.2, 0.933], [0.577, -0.577, 0.577]], F32)


def frame_normals():
    e = F32(0.99)
    out = [SPECIAL_NORMALS]
    for x in (e, np.nextafter(e, F32(2)), np.nextafter(e, F32(0))):
        y = np.sqrt(max(0.0, 1 - float(x) ** 2))
        out.append(np.array([[x, y, 0], [-x, 0, y]], F32))
    rng = np.random.default_rng(5)
    n = unit_normals(8, rng)
    out += [n * F32(1.7), n * F32(0.3)]
    return np.concatenate(out, 0)


def roughness_cases(S=16, ceps=1e-14):
    out = []
    for k, r in enumerate((0.0, 0.01, 0.8, 1.0)):
        c = smooth_case(48, S, seed=20 + k, family="B", name="B_r=%g_S%d" % (r, S), ceps=ceps)
        c.rough[:] = r
        c.smooth = False
        out.append(c)
    for k, (lo, hi) in enumerate(((0.001, 0.02), (0.02, 0.06), (0.9, 1.0))):
        c = smooth_case(96, S, seed=30 + k, rlo=lo, rhi=hi, family="B", name="B_r[%g,%g]_S%d" % (lo, hi, S), ceps=ceps)
        c.smooth = lo >= 0.9
        out.append(c)
    return out


def frame_cases(S=16):
    n = frame_normals()
    rng = np.random.default_rng(41)
    P = len(n)
    nn = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-9)
    pts = front_points(nn.astype(F32), rng)
    return [Case("C_frames_S%d" % S, "C", n, rng.uniform(0.1, 0.7, P), pts, CAM, rng.random((P, 2), F32), S, 41, named=())]   # (the axis choice is exact: never uncertain)


def view_cases(S=16):
    rng = np.random.default_rng(43)
    out = []
    n = unit_normals(24, rng)
    r = rng.uniform(0.1, 0.7, 24)
    sh = rng.random((24, 2), F32)
    # behind the surface: ndv = 0
    out.append(Case("D_behind_S%d" % S, "D", n, r, CAM[None] + n * 1.5 + 0.1 * rng.normal(size=(24, 3)), CAM, sh, S, 43, named=("ndv_lo",)))
    # grazing: view direction t * cos + n * sin with sin = 1e-3 .. 1e-7 (both clamp_eps)
    t = np.cross(n, np.roll(n, 1, 0))
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    g = 10.0 ** -rng.uniform(3, 7, (24, 1))
    d = t * np.sqrt(1 - g * g) + n * g
    for ce in (1e-14, 1e-6):
        out.append(Case("D_grazing_ceps%g_S%d" % (ce, S), "D", n, r, CAM[None] - d * 2.0, CAM, sh, S, 44, ceps=ce, named=("ndv_lo", "den_b_lo", "ndl_lo")))
    out.append(Case("D_along_normal_S%d" % S, "D", n, r, CAM[None] - n * 1.25, CAM, sh, S, 45, named=("ndv_hi", "ndh_hi", "vdh_hi")))
    # at the point and 5e-5 away from it: the eps = 1e-4 floor of F.normalize
    pts = np.repeat(CAM[None], 24, 0).astype(np.float64)
    pts[12:] -= n[12:] * 5e-5
    out.append(Case("D_at_camera_S%d" % S, "D", n, r, pts, CAM, sh, S, 46, named=("lv_lo", "ndv_lo")))
    return out


def shift_cases(S=16):
    rng = np.random.default_rng(47)
    ham = MS.hammersley_points(S)
    out = []
    P = 30
    n = unit_normals(P, rng)
    r = rng.uniform(0.1, 0.7, P)
    pts = front_points(n, rng)
    sh = np.zeros((P, 2), F32)                                   # rows 0-5: shift 0
    one = F32(1.0)
    for j in range(6, 18):                                       # ham + shift = 1 exactly (not wrapped) and the float32 neighbours of that shift
        i, k = (j * 5) % S, j % 2                                # (one coordinate per pixel, the other one random: at most a few kinks per sample)
        base = one - ham[i, k]
        sh[j] = rng.random(2)
        sh[j, k] = (base, np.nextafter(base, F32(2)), np.nextafter(base, F32(-1)))[(j // 2) % 3]
    sh[18:22] = (np.nextafter(one, F32(0)), 5e-7)                # sums that clamp at both ends: 1 - ulp + 0 -> upper clamp; wrapped to < 1e-6 -> lower clamp
    sh[22:26, 0] = rng.random(4)
    sh[22:26, 1] = (0.0, 0.5, 1.0, 0.25)                         # s1 -> phi = -pi (clamped 1e-6), 0, pi
    sh[26:] = (1.0, 1.0)                                         # every sum but the first wraps
    out.append(Case("E_shifts_S%d" % S, "E", n, r, pts, CAM, sh, S, 47, named=DISC[1:] + ("s0_lo", "s0_hi", "s1_lo", "s1_hi", "ct_hi", "st_hi", "ndh_hi")))
    return out


def light_cases(S=16):
    out = []
    for k, (light, grad) in enumerate((("zeros", "random"), ("onehot", "random"), ("lamp", "random"), ("random", "zeros"), ("random", "channel"))):
        out.append(smooth_case(37, S, seed=60 + k, family="F", name="F_%s_%s_S%d" % (light, grad, S), light=light, grad=grad))
    return out


def shape_cases(S):
    """family A at one S, P around the pixels per wave; clamp_eps alternates"""
    return [smooth_case(P, S, seed=1, ceps=1e-6 if P % 2 == 0 else 1e-14) for P in p_list(S)]


GRID_CAP_SHAPES = [(16, 3 * 32 + 7), (100, 3 * 8 + 3), (1, 3 * 512 + 77)]      # (S, P): with TEXIR_SPEC_GRID_CAP = 2, three full rounds and a partial one
LPP_SHAPES = [(lpp, S) for lpp in (1, 4, 16) for S in (16, 24, 100)]


def grid_cap_case(S, P):
    return smooth_case(P, S, seed=2)


def lpp_cases(lpp, S):
    ppw = 64 // lpp
    return [smooth_case(P, S, seed=3, ceps=1e-6 if lpp == 4 else 1e-14) for P in (ppw - 1, 4 * ppw + 1)]


def autograd_case():
    return smooth_case(37, 24, seed=4)


def family_cases():
    out = []
    for S in (16, 100):
        out += roughness_cases(S)
    out += roughness_cases(24, ceps=1e-6)
    out += frame_cases(16) + frame_cases(65) + view_cases(16) + view_cases(24) + shift_cases(16) + shift_cases(100) + light_cases(16) + light_cases(63)
    return out


# ---- float32 implementations and mutants (CPU) -------------------------------------------------------------------------------------------------------

def chain_f32(case, mut=None, dual=True):
    """the chain op by op in torch float32 -> (w [M], dw [M], l [M,3]); dual=False: dw by float32 autograd"""
    inp = case.inputs(torch.float32)
    if not dual:
        inp["r"].requires_grad_(True)
    ch = Chain(inp, case.ceps, Tape(on=False), mut=mut, dual=dual)
    w, l = ch.spec()
    if dual:
        dw = torch.zeros_like(w.v) if w.d is None else w.d
    else:
        dw, = torch.autograd.grad(w.v.sum(), inp["r"])
    f = lambda x: x.detach().double().numpy()[:, 0]
    return f(w.v), f(dw), np.stack([f(x.v) for x in l], -1)


def pixel_f32(case, w, dw, mut=None):
    """the per-pixel stage in float32 on per-sample weights -> rgb, d_albedo, d_rough"""
    P, S = case.P, case.S
    t = lambda x: torch.from_numpy(np.asarray(x, F32))
    w, dw = t(w).reshape(P, S, 1), t(dw).reshape(P, S)
    L, g, irr, alb = t(case.L), t(case.d_rgb), t(case.irr), t(case.albedo)
    div = 64.0 if mut == "inv_S_is_64" else float(S)
    pi = F32(math.pi).item()
    rgb = irr * alb / pi + (L * w).sum(1) / div
    d_alb = g * irr if mut == "dalbedo_no_pi" else g * irr / pi
    d_r = ((L * g[:, None, :]).sum(-1) * dw).sum(1) / div
    return rgb.double().numpy(), d_alb.double().numpy(), d_r.double().numpy()
