"""Reference, error bound and case matrix of the optimiser kernels (csrc/adam.hip: adam_kernel, adam_tex_kernel<C>, adam_tex_vec_kernel<C>,
adam_tex_vec_batch_kernel<CSET>, adam_tick_kernel; csrc/material.hip: grad_add_masked_kernel).  numpy only, no GPU.

Reference: the float32 arrays and float32 scalars exactly as the C ABI receives them, every operation evaluated in float64:
    g1c = 0.25 g2 + g1,  g = 0.25 g1c + g0          (texture forms; a gradient reads as zero where its pointer is NULL or its mask bit is clear)
    m' = (g - m)(1 - b1) + m,  v' = g^2 (1 - b2) + v b2
    den = sqrt(v') / bc2_sqrt + eps,  p' = clamp(p - step_size m' / den)
    mip1 = 0.25 (((p00 + p01) + p10) + p11)          of the updated, clamped texels
(step_size, bc2_sqrt) is the float32 pair the kernel reads (`hyper`), or, for the forms that take (lr, step), the float32 rounding of
lr / (1 - beta1^step) and sqrt(1 - beta2^step) computed in float64 from the float32 betas, with one extra u of relative error allowed on each.

Bound: a first-order running error analysis of exactly that sequence, one line per rounded operation, computed in float64 from reference values only
(u = 2^-24, eta = 2^-126 per operation so that neither gradual underflow nor a flush could matter):
    e(g1c) = u|g1c| + eta
    e(g)   = 0.25 e(g1c) + u|g| + eta                 (flat kernel: e(g) = 0)
    e(d)   = e(g) + u|g - m| + eta
    e(m')  = (1-b1) e(d) + u|m'| + eta
    e(s)   = 2|g| e(g) + u g^2 + eta
    e(t)   = u v b2 + eta
    e(v')  = (1-b2) e(s) + e(t) + u v' + eta
    e(r)   = sqrt(v' + e(v')) - sqrt(max(v' - e(v'), 0)) + u r + eta        (r = sqrt(v'))
    e(q)   = e(r)/bc + u q + eta                      (q = r/bc)
    e(den) = e(q) + u den + eta
    e(z)   = e(m')/(den - e(den)) + |m'| e(den)/(den (den - e(den))) + u|z| + eta     (z = m'/den)
    e(p')  = step_size e(z) + u|p'_unclamped| + eta   (clamp is 1-Lipschitz: no extra term)
    e(mip1)= 0.25 (sum of the four e(p')) + 0.25 u(|s1| + |s2| + |s3|) + eta          (the three partial sums)
An output passes when |got - ref| <= K e with K = 2, fixed before any run: K covers the second-order terms, the float64 evaluation itself and a
faithfully rather than correctly rounded sqrt.  Every case must satisfy e(den) < den/2 and have finite reference values: asserted in the reference.

tests/test_adam_ref_cpu.py proves this checker without a GPU (an op-by-op float32 emulation passes, operator mutants are rejected);
tests/test_gpu_adam_kernels.py runs the kernels through it.
"""
import itertools

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126
K = 2.0
F32 = np.float32
F64 = np.float64

FAMILIES = ("typical", "fresh", "zerograd", "spread", "cancel")
NONZERO = tuple(f for f in FAMILIES if f != "zerograd")
CLAMPS = ((1e-2, 0.8), (0.0, np.inf), (-np.inf, np.inf))
EPSS = (1e-8, 1e-3)
STEPS = (1, 3, 1000)
SETTINGS = tuple(itertools.product(FAMILIES, CLAMPS, EPSS, STEPS))                      # 90
SETTINGS_NZ = tuple(s for s in SETTINGS if s[0] != "zerograd")                          # 72
MASK_PATTERNS = ("none", "all", "half", "bit0", "bit31", "bit32", "last")
LR = 3e-2

RATIOS = {}          # (entry point, family) -> {output: worst error / e} (test_zz_record prints it)


# ------------------------------------------------------------------------------------------------------------------
# masks: bit t = y * W + x, LSB first in uint32 words, ceil(n / 32) words (the level-1 mask: the same over the half-resolution grid)
# ------------------------------------------------------------------------------------------------------------------
def pack_mask(bits):
    bits = np.asarray(bits, bool).ravel()
    b = np.zeros(((bits.size + 31) // 32) * 32, np.uint8)
    b[:bits.size] = bits
    return np.ascontiguousarray(np.packbits(b.reshape(-1, 32), axis=1, bitorder="little")).view("<u4").ravel().copy()


def unpack_mask(words, n):
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def mask_bits(pattern, n, rng):
    b = np.zeros(n, bool)
    if pattern == "all":
        b[:] = True
    elif pattern == "half":
        b = rng.random(n) < 0.5
    elif pattern == "last":
        b[n - 1] = True
    elif pattern.startswith("bit"):
        b[int(pattern[3:])] = True           # (callers skip a pattern whose bit lies past the last texel)
    else:
        assert pattern == "none"
    return b


def pattern_fits(pattern, n):
    return not (pattern.startswith("bit") and int(pattern[3:]) >= n)


# ------------------------------------------------------------------------------------------------------------------
# the step size / bias correction of the forms that take (lr, step)
# ------------------------------------------------------------------------------------------------------------------
def host_hyper(lr, b1, b2, step):
    lr, b1, b2 = F64(F32(lr)), F64(F32(b1)), F64(F32(b2))
    return F32(lr / (1.0 - b1 ** F64(step))), F32(np.sqrt(1.0 - b2 ** F64(step)))


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
class Case:
    """one call: H is None for the flat kernel (p, g0, m, v one-dimensional), else a texture [H, W, C].  All arrays float32 (masks uint32 words)."""

    def __init__(self, **kw):
        self.H = self.W = self.C = None
        self.g0 = self.mask0 = self.g1 = self.mask1 = self.g2 = None
        self.mip = False
        self.__dict__.update(kw)

    @property
    def form(self):
        if self.H is None:
            return ("flat",)
        return (self.group, "null" if self.g0 is None else "masked" if self.mask0 is not None else "dense", self.g1 is not None,
                self.mask1 is not None, self.g2 is not None, self.mip)


def _up2(a):
    return a.repeat(2, axis=0).repeat(2, axis=1)


def _grad(rng, family, shape):
    if family == "zerograd":
        return np.zeros(shape, F32)
    if family == "spread":
        return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-12, 4, shape)).astype(F32)
    return (rng.standard_normal(shape) * 0.5).astype(F32)


def _state(rng, family, shape, gfold):
    p = rng.uniform(-0.1, 1.0, shape).astype(F32)
    if family == "spread":
        m = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-12, 4, shape)).astype(F32)
        v = (10.0 ** rng.uniform(-24, 8, shape)).astype(F32)
    else:
        m = (rng.standard_normal(shape) * 0.2).astype(F32)
        v = (rng.uniform(0, 1e-3, shape)).astype(F32)
    if family == "fresh":
        m[...] = 0
        v[...] = 0
    if family == "zerograd":
        v[...] = 0
    if family == "cancel":
        m = (gfold * (1.0 + rng.integers(-4, 5, shape) * 2.0 ** -22)).astype(F32)
    return p, m, v


def _hyper_fields(setting, lr, betas):
    family, (lo, hi), eps, step = setting
    b1, b2 = F32(betas[0]), F32(betas[1])
    ss, bc = host_hyper(lr, b1, b2, step)
    return dict(family=family, lo=F32(lo), hi=F32(hi), eps=F32(eps), step=int(step), lr=F32(lr), b1=b1, b2=b2, ss=ss, bc=bc)


def flat_case(n, setting, seed, lr=LR, betas=(0.9, 0.999)):
    rng = np.random.default_rng(seed)
    g = _grad(rng, setting[0], (n,))
    p, m, v = _state(rng, setting[0], (n,), g.astype(F64))
    return Case(group="flat", n=n, p=p, g0=g, m=m, v=v, **_hyper_fields(setting, lr, betas))


def tex_case(group, H, W, C, g0mode, g1, g2, mip, setting, seed, pattern="half", mask1=None, lr=LR, betas=(0.9, 0.999)):
    """g0mode: 'dense' | 'masked' | 'null'; g1 / g2 / mip: given or NULL; mask1: pattern of the level-1 mask (batched form, needs g2) or None"""
    assert g1 or g2
    assert not g2 or (H % 4 == 0 and W % 4 == 0)
    assert mask1 is None or (g1 and g2)
    rng = np.random.default_rng(seed)
    fam = setting[0]
    Hh, Wh = H // 2, W // 2
    c = Case(group=group, H=H, W=W, C=C, mip=bool(mip), **_hyper_fields(setting, lr, betas))
    nan = F32(np.nan)
    fold1 = np.zeros((Hh, Wh, C))
    if g1:
        c.g1 = _grad(rng, fam, (Hh, Wh, C))
        if mask1 is not None:
            bits = mask_bits(mask1, Hh * Wh, rng)
            c.mask1 = pack_mask(bits)
            c.g1[~bits.reshape(Hh, Wh)] = nan                         # a never-cleared buffer: not to be read where the bit is clear
        fold1 = np.where(np.isnan(c.g1), 0.0, c.g1.astype(F64))
    if g2:
        c.g2 = _grad(rng, fam, (H // 4, W // 4, C))
        fold1 = 0.25 * _up2(c.g2.astype(F64)) + fold1
    fold0 = 0.25 * _up2(fold1)
    if g0mode != "null":
        c.g0 = _grad(rng, fam, (H, W, C))
        if g0mode == "masked":
            bits = mask_bits(pattern, H * W, rng)
            c.mask0 = pack_mask(bits)
            c.g0[~bits.reshape(H, W)] = nan
        fold0 = fold0 + np.where(np.isnan(c.g0), 0.0, c.g0.astype(F64))
    c.p, c.m, c.v = _state(rng, fam, (H, W, C), fold0)
    return c


# ------------------------------------------------------------------------------------------------------------------
# the float64 reference and its bound
# ------------------------------------------------------------------------------------------------------------------
def _bits_or_all(words, n):
    return np.ones(n, bool) if words is None else unpack_mask(words, n)


def folded_gradient(c):
    """(g, e(g)) of a case in float64"""
    if c.H is None:
        g = c.g0.astype(F64)
        return g, np.zeros_like(g)
    H, W, C = c.H, c.W, c.C
    Hh, Wh = H // 2, W // 2
    g1 = np.zeros((Hh, Wh, C))
    if c.g1 is not None:
        g1 = np.where(_bits_or_all(c.mask1, Hh * Wh).reshape(Hh, Wh, 1), c.g1.astype(F64), 0.0)
    g1c = g1 if c.g2 is None else 0.25 * _up2(c.g2.astype(F64)) + g1
    e1 = U * np.abs(g1c) + ETA
    g0 = np.zeros((H, W, C))
    if c.g0 is not None:
        g0 = np.where(_bits_or_all(c.mask0, H * W).reshape(H, W, 1), c.g0.astype(F64), 0.0)
    g = 0.25 * _up2(g1c) + g0
    return g, 0.25 * _up2(e1) + U * np.abs(g) + ETA


def reference(c, extra_u=0):
    """{'p', 'm', 'v', 'mip1'}: (value, e) in float64 ('mip1' None for the flat kernel and where mip_level1 is NULL).  extra_u: additional relative error
    (in u) of step_size and bc2_sqrt, 1 for the forms that compute the pair themselves from (lr, step)"""
    g, eg = folded_gradient(c)
    p, m, v = c.p.astype(F64), c.m.astype(F64), c.v.astype(F64)
    b1, b2, eps, ss, bc, lo, hi = (F64(x) for x in (c.b1, c.b2, c.eps, c.ss, c.bc, c.lo, c.hi))
    with np.errstate(all="raise", under="ignore"):
        d = g - m
        ed = eg + U * np.abs(d) + ETA
        m1 = d * (1 - b1) + m
        em = (1 - b1) * ed + U * np.abs(m1) + ETA
        es = 2 * np.abs(g) * eg + U * g * g + ETA
        et = U * v * b2 + ETA
        v1 = g * g * (1 - b2) + v * b2
        ev = (1 - b2) * es + et + U * v1 + ETA
        r = np.sqrt(v1)
        er = np.sqrt(v1 + ev) - np.sqrt(np.maximum(v1 - ev, 0)) + U * r + ETA
        q = r / bc
        eq = er / bc + U * q + ETA + extra_u * U * q
        den = q + eps
        eden = eq + U * den + ETA
        assert (eden < den / 2).all(), "case outside the bound's domain: e(den) >= den/2"
        z = m1 / den
        ez = em / (den - eden) + np.abs(m1) * eden / (den * (den - eden)) + U * np.abs(z) + ETA
        pu = p - ss * z
        ep = ss * ez + U * np.abs(pu) + ETA + extra_u * U * ss * np.abs(z)
        p1 = np.minimum(np.maximum(pu, lo), hi)
    out = {"p": (p1, ep), "m": (m1, em), "v": (v1, ev), "mip1": None}
    if c.H is not None and c.mip:
        P = p1.reshape(c.H // 2, 2, c.W // 2, 2, c.C)
        E = ep.reshape(c.H // 2, 2, c.W // 2, 2, c.C)
        s1 = P[:, 0, :, 0] + P[:, 0, :, 1]
        s2 = s1 + P[:, 1, :, 0]
        s3 = s2 + P[:, 1, :, 1]
        out["mip1"] = (0.25 * s3, 0.25 * E.sum(axis=(1, 3)) + 0.25 * U * (np.abs(s1) + np.abs(s2) + np.abs(s3)) + ETA)
    for k, ve in out.items():
        assert ve is None or (np.isfinite(ve[0]).all() and np.isfinite(ve[1]).all() and (ve[1] > 0).all()), "non-finite reference (%s)" % k
    return out


def ratios(ref, got):
    """worst |got - ref| / e per output (inf: non-finite output, a missing output or a wrong shape)"""
    out = {}
    for k, ve in ref.items():
        if ve is None:
            continue
        a = got.get(k)
        if a is None or a.shape != ve[0].shape or a.dtype != F32 or not np.isfinite(a).all():
            out[k] = np.inf
            continue
        out[k] = float((np.abs(a.astype(F64) - ve[0]) / ve[1]).max()) if a.size else 0.0
    return out


def accepts(ref, got):
    return all(r <= K for r in ratios(ref, got).values())


def check_outputs(ref, got, tag=None, what=""):
    """asserts every element of every output inside K e and keeps the worst ratio under `tag` = (entry point, family)"""
    rs = ratios(ref, got)
    if tag is not None:
        rec = RATIOS.setdefault(tag, {})
        for k, r in rs.items():
            rec[k] = max(rec.get(k, 0.0), r)
    for k, r in rs.items():
        if not r <= K:
            a, (val, e) = got[k], ref[k]
            msg = "%s %s: output %s " % (tag, what, k)
            if a is None or a.shape != val.shape or not np.isfinite(a).all():
                raise AssertionError(msg + "missing, misshapen or non-finite")
            i = np.unravel_index(np.argmax(np.abs(a.astype(F64) - val) / e), val.shape)
            raise AssertionError(msg + "element %s: got %.9g, reference %.17g, error / e = %.3f > K = %g" % (i, a[i], val[i], r, K))
    return rs


# ------------------------------------------------------------------------------------------------------------------
# grad_add_masked: g += g0 where the texel's bit is set -- one rounded add
# ------------------------------------------------------------------------------------------------------------------
def grad_add_case(n_texels, C, pattern, family, seed):
    rng = np.random.default_rng(seed)
    bits = mask_bits(pattern, n_texels, rng)
    g = _grad(rng, "typical" if family == "zerograd" else family, (n_texels, C))
    g0 = _grad(rng, family, (n_texels, C))
    if n_texels:
        g.ravel()[::7] = F32(-0.0)                                    # (a texel whose bit is clear keeps its bits: the sign of a zero too)
    g0[~bits] = F32(np.nan)
    return Case(group="grad_add", n=n_texels, C=C, g=g, g0=g0, bits=bits, mask=pack_mask(bits), family=family)


def check_grad_add(c, got, tag=None):
    """got: g after the call"""
    assert got.shape == c.g.shape and got.dtype == F32
    on = np.broadcast_to(c.bits[:, None], c.g.shape)
    assert (got[~on].view(np.uint32) == c.g[~on].view(np.uint32)).all(), "an element whose mask bit is clear changed its bits"
    s = c.g[on].astype(F64) + c.g0[on].astype(F64)
    assert np.isfinite(s).all() and np.isfinite(got[on]).all()
    r = float((np.abs(got[on].astype(F64) - s) / (U * np.abs(s) + ETA)).max()) if s.size else 0.0
    if tag is not None:
        rec = RATIOS.setdefault(tag, {})
        rec["g"] = max(rec.get("g", 0.0), r)
    assert r <= K, "grad_add_masked: error / e = %.3f > K" % r
    return r


# ------------------------------------------------------------------------------------------------------------------
# adam_tick: step' = step + 1, hyper = (lr / (1 - b1^step'), sqrt(1 - b2^step')) from the record's doubles, at 60 digits
# ------------------------------------------------------------------------------------------------------------------
def tick_exact(step, lr, b1, b2):
    """(step', step_size, bc2_sqrt) of one record (float64 inputs, taken exactly), the pair as mpmath numbers"""
    import mpmath
    with mpmath.workprec(200):                                        # 60 digits
        s = mpmath.mpf(float(step)) + 1
        lr, b1, b2 = (mpmath.mpf(float(x)) for x in (lr, b1, b2))
        return float(s), +(lr / (1 - b1 ** s)), +mpmath.sqrt(1 - b2 ** s)


def _f32_round(x):
    """float32 nearest to an mpmath number (through the nearest double: a double rounding can only matter at a tie, which the neighbours cover)"""
    return F32(float(x))


def tick_allowed(x):
    """the float32 rounding of an exact value and that rounding's two float32 neighbours"""
    r = _f32_round(x)
    return (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf)))


def check_tick(state0, hyper0, mask, state1, hyper1):
    """state [n][4] float64 (step, lr, beta1, beta2), hyper [n][2] float32, before and after one tick with `mask`"""
    n = state0.shape[0]
    assert state1.shape == state0.shape and hyper1.shape == hyper0.shape
    for i in range(n):
        if not (mask >> i) & 1:
            assert (state1[i].view(np.uint64) == state0[i].view(np.uint64)).all() and (hyper1[i].view(np.uint32) == hyper0[i].view(np.uint32)).all(), \
                "record %d is not selected and changed" % i
            continue
        s, ss, bc = tick_exact(*state0[i])
        assert state1[i, 0] == s, "record %d: step %r, expected %r" % (i, state1[i, 0], s)
        assert (state1[i, 1:].view(np.uint64) == state0[i, 1:].view(np.uint64)).all(), "record %d: lr / betas changed" % i
        assert hyper1[i, 0] in tick_allowed(ss), "record %d: step_size %r, exact %s" % (i, hyper1[i, 0], ss)
        assert hyper1[i, 1] in tick_allowed(bc), "record %d: bc2_sqrt %r, exact %s" % (i, hyper1[i, 1], bc)


TICK_BETAS = ((0.9, 0.999), (float(F32(0.9)), float(F32(0.999))), (0.0, 0.0))
TICK_STEPS = (0.0, 9.0, 1e5 - 1, 1e7 - 1)
TICK_N = (0, 1, 3, 64)


def tick_masks(n):
    full = (1 << n) - 1 if n else 0
    return sorted({0, full, 0x5555555555555555 & full, (1 << 63) & full})


def tick_state(n, seed):
    """n records cycling through every (step, betas) pair of the matrix, learning rates all different"""
    combos = list(itertools.product(TICK_STEPS, TICK_BETAS))
    st = np.zeros((n, 4), F64)
    for i in range(n):
        s, (b1, b2) = combos[(i + seed) % len(combos)]
        st[i] = (s, 3e-2 / (1 + i), b1, b2)
    hy = np.full((n, 2), -3.0, F32) + np.arange(2 * n, dtype=F32).reshape(n, 2)
    return st, hy


# ------------------------------------------------------------------------------------------------------------------
# op-by-op float32 emulation of the kernels (the CPU stand-in that proves the checker), with operator mutants
# ------------------------------------------------------------------------------------------------------------------
MUTANTS = ("omb2_decimal", "eps_in_root", "no_bias", "no_clamp", "mask_shift", "l2_axis", "fold1_half", "fold0_half")
LEGIT = ("two_rounding_m",)


def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _emu_bits(words, n, mut):
    if words is None:
        return np.ones(n, bool)
    b = unpack_mask(words, n)
    return np.roll(b, -1) if mut == "mask_shift" else b              # bit t + 1 read for texel t


def _emu_read(a, bits):
    return np.where(bits, a, F32(0))


def emulate(c, mut=None):
    """the kernels' float32 operation sequence in numpy (fused multiply-add through a float64 product and sum)"""
    with np.errstate(all="ignore"):
        if c.H is None:
            g = c.g0
        else:
            H, W, C = c.H, c.W, c.C
            Hh, Wh = H // 2, W // 2
            g1c = np.zeros((Hh, Wh, C), F32)
            if c.g1 is not None:
                g1c = _emu_read(c.g1, _emu_bits(c.mask1, Hh * Wh, mut).reshape(Hh, Wh, 1))
            if c.g2 is not None:
                if mut == "l2_axis":                                  # row from the column index and the reverse
                    by, bx = np.meshgrid(np.arange(Hh), np.arange(Wh), indexing="ij")
                    x2 = c.g2[(bx >> 1) % (H // 4), (by >> 1) % (W // 4)]
                else:
                    x2 = _up2(c.g2)
                g1c = _fma(F32(0.5 if mut == "fold1_half" else 0.25), x2, g1c)
            g0 = np.zeros((H, W, C), F32)
            if c.g0 is not None:
                g0 = _emu_read(c.g0, _emu_bits(c.mask0, H * W, mut).reshape(H, W, 1))
            g = _fma(F32(0.5 if mut == "fold0_half" else 0.25), _up2(g1c), g0)
        one = F32(1)
        omb1, omb2 = one - c.b1, one - c.b2
        if mut == "omb2_decimal":
            omb2 = F32(1.0 - float("%.6g" % c.b2))                    # 0.001f in the place of 1 - 0.999f
        if mut == "two_rounding_m":
            mi = c.m * c.b1 + g * omb1
        else:
            mi = _fma(g - c.m, omb1, c.m)
        vi = _fma(g * g, omb2, c.v * c.b2)
        bc = one if mut == "no_bias" else c.bc
        if mut == "eps_in_root":
            den = np.sqrt(vi + c.eps) / bc
        else:
            den = np.sqrt(vi) / bc + c.eps
        pi = _fma(mi / den, -c.ss, c.p)
        if mut != "no_clamp":
            pi = np.minimum(np.maximum(pi, c.lo), c.hi)
        out = {"p": pi.astype(F32), "m": mi.astype(F32), "v": vi.astype(F32), "mip1": None}
        if c.H is not None and c.mip:
            P = out["p"].reshape(Hh, 2, Wh, 2, C)
            out["mip1"] = F32(0.25) * (((P[:, 0, :, 0] + P[:, 0, :, 1]) + P[:, 1, :, 0]) + P[:, 1, :, 1])
    return out


def mutant_applies(mut, c):
    """whether a mutant changes the operation at all for this case's form (a zero-gradient case cannot see one that only changes how the gradient enters)"""
    if mut == "no_clamp":
        return bool(np.isfinite(c.lo) or np.isfinite(c.hi))
    if mut == "mask_shift":
        return c.mask0 is not None or c.mask1 is not None
    if mut in ("l2_axis", "fold1_half"):
        return c.g2 is not None and (mut != "l2_axis" or c.g2.shape[0] * c.g2.shape[1] > 1)
    if mut == "fold0_half":
        return c.H is not None
    return True


# ------------------------------------------------------------------------------------------------------------------
# the matrix.  A spec is the argument tuple of flat_case / tex_case; cases are built one at a time.
# adam_vec_epb = 960 floats for C = 3, 1024 otherwise
# ------------------------------------------------------------------------------------------------------------------
FLAT_N = (0, 1, 255, 256, 257, 4096 * 256 + 257)
VEC_SHAPES = ((2, 2, 2), (2, 4, 1), (4, 4, 3), (6, 320, 3), (4, 324, 3), (8, 644, 3), (4, 1028, 1), (4, 516, 2), (4, 260, 4), (4100, 4, 1))
GRID_Y_SHAPE, GRID_Y = (20, 324, 3), 3
SCALAR_SHAPES = ((2, 2, 1), (6, 6, 3), (4, 342, 3), (8196, 2, 1))
FORCED_SCALAR_SHAPES = ((4, 324, 3), (8, 644, 3))
CROSS_SHAPES = ((4, 324, 3), (2, 2, 2))


def pointer_combos(H, W, dev=True):
    """every (g0mode, g1, g2, mip) the argument checks allow: level 2 needs H and W divisible by 4, the forms that take (lr, step) need level 1"""
    out = []
    for g0mode, g1, g2, mip in itertools.product(("dense", "masked", "null"), (True, False), (True, False), (True, False)):
        if (not g1 and not g2) or (g2 and (H % 4 or W % 4)) or (not g1 and not dev):
            continue
        out.append((g0mode, g1, g2, mip))
    return out


def covering_combos(H, W):
    """a subset of pointer_combos in which every pointer state occurs at least once"""
    if H % 4 or W % 4:
        return [("dense", True, False, True), ("masked", True, False, False), ("null", True, False, True)]
    return [("dense", True, True, True), ("masked", False, True, False), ("null", True, False, True), ("masked", True, True, True)]


def _nz(i):
    return SETTINGS_NZ[(i * 37) % len(SETTINGS_NZ)]


def flat_specs():
    """(n, setting, seed): the whole settings matrix at n = 257, a rotation elsewhere (every non-empty n with a non-zero gradient)"""
    out = [(257, s, 100 + i) for i, s in enumerate(SETTINGS)]
    for j, n in enumerate(FLAT_N):
        out += [(n, _nz(j), 300 + j)] + ([(n, SETTINGS[(j * 41 + 20) % len(SETTINGS)], 320 + j)] if n < 1000 else [])
    return out


def tex_specs(group):
    """argument tuples of tex_case for one group of the matrix: 'vector' | 'grid_y' | 'scalar' | 'forced_scalar' | 'cross' | 'settings' | 'patterns'"""
    out = []
    seed = itertools.count({"vector": 1000, "grid_y": 2000, "scalar": 3000, "forced_scalar": 4000, "cross": 5000, "settings": 6000, "patterns": 7000}[group])
    if group in ("vector", "scalar", "forced_scalar", "grid_y"):
        shapes = {"vector": VEC_SHAPES, "scalar": SCALAR_SHAPES, "forced_scalar": FORCED_SCALAR_SHAPES, "grid_y": (GRID_Y_SHAPE,)}[group]
        i = 0
        for (H, W, C) in shapes:
            for (g0mode, g1, g2, mip) in covering_combos(H, W):
                i += 1
                pat = MASK_PATTERNS[i % len(MASK_PATTERNS)]
                out.append((group, H, W, C, g0mode, g1, g2, mip, _nz(i + len(shapes)), next(seed), pat if pattern_fits(pat, H * W) else "half"))
    elif group == "cross":
        i = 0
        for (H, W, C) in CROSS_SHAPES:
            for (g0mode, g1, g2, mip) in pointer_combos(H, W):
                i += 1
                out.append((group, H, W, C, g0mode, g1, g2, mip, _nz(i), next(seed), "half"))
                out.append((group, H, W, C, g0mode, g1, g2, mip, SETTINGS[(i * 41) % len(SETTINGS)], next(seed), "half"))
    elif group == "settings":                                            # the whole settings matrix on one shape and combination
        for s in SETTINGS:
            out.append((group, 4, 324, 3, "masked", True, True, True, s, next(seed), "half"))
    elif group == "patterns":
        i = 0
        for (H, W, C) in CROSS_SHAPES + ((4, 4, 3),):
            for pat in MASK_PATTERNS:
                if pattern_fits(pat, H * W):
                    i += 1
                    out.append((group, H, W, C, "masked", True, H % 4 == 0, True, _nz(i), next(seed), pat))
    return out


TEX_GROUPS = ("vector", "grid_y", "scalar", "forced_scalar", "cross", "settings", "patterns")

# the batches: (H, W, C, g0mode, g1, g2, mip, level-1 mask pattern) per job.  Jobs differ in H (gy 2 and 10 row pairs... 4 and 20 rows), one job has several
# row segments (so `first` > 1 for the jobs behind it), one has a level1_mask, every job its own hyper pair, betas, eps and clamps.
_J_A = (4, 324, 3, "masked", True, True, True, "half")                   # two segments, level1_mask
_J_B = (20, 8, 3, "dense", True, True, True, None)
_J_C = (20, 1028, 1, "null", True, True, True, "half")                   # two segments
_J_D = (4, 8, 1, "masked", False, True, False, None)
_J_E = (4, 516, 2, "dense", True, False, True, None)                     # two segments
_J_F = (20, 4, 4, "masked", True, True, False, "bit0")
_J_S = (2, 2, 1, "dense", True, False, True, None)                       # cannot take the vector form: the whole batch takes the scalar launches
BATCHES = {
    "c3_n1": (_J_A,),
    "c3_n2": (_J_A, _J_B),
    "c1_n2": (_J_C, _J_D),
    "c13_n3": (_J_C, _J_A, _J_D),
    "c13_n4": (_J_A, _J_C, _J_B, _J_D),
    "c2431_n4": (_J_E, _J_F, _J_A, _J_D),
    "c2431_n4_rev": (_J_D, _J_A, _J_F, _J_E),
    "scalar_n3": (_J_A, _J_S, _J_C),
}
_JOB_BETAS = ((0.9, 0.999), (0.8, 0.99), (0.95, 0.995), (0.85, 0.9999))
_JOB_LR = (3e-2, 1e-2, 5e-3, 7e-2)


def batch_cases(name, variant=0):
    """the cases of one batch; variant shifts the settings rotation"""
    out = []
    for k, (H, W, C, g0mode, g1, g2, mip, m1) in enumerate(BATCHES[name]):
        out.append(tex_case("batch", H, W, C, g0mode, g1, g2, mip, _nz(11 * variant + 5 * k + len(name)), 9000 + 10 * variant + k + 100 * sorted(BATCHES).index(name),
                            pattern="half", mask1=m1, lr=_JOB_LR[k], betas=_JOB_BETAS[k]))
    return out
