"""Float64 restatement of the texture fetch (wrap-bilinear / trilinear over a 2x2-box mip chain) as an EXPLICIT LINEAR OPERATOR, the float32
rounding model its comparisons are bounded by, check(), the seeded case generators and the mutants the checker must reject.  Shared by
test_texture_ref_cpu.py (no GPU) and test_gpu_texture_kernels.py (no tests here).

Semantics restated from the documentation of the operator, not from the kernels:
  * boundary mode wrap: only the fractional part of u, v counts; texel i of a W-wide level has its centre at (i + 0.5) / W;
  * the mip chain halves both sides by a 2x2 box while both are even, for at most max_mip_level levels above level 0 (16 levels in all);
  * with the footprint J = [[du/dX * W, du/dY * W], [dv/dX * H, dv/dY * H]] (texels of level 0 per pixel), the level is
    clamp(0.5 * log2(major), 0, levels - 1), major = the larger eigenvalue of J^T J = the squared major axis of the footprint ellipse;
  * trilinear = blend of the bilinear samples of floor(level) and the next level.

Everything is numpy float64 on float32 inputs; nothing is ever rounded to float32.

THE BOUND.  u = 2^-24 is the unit roundoff of float32.  Every compared element gets bound = K * (accumulation + coordinate + level):
  accumulation  n_roundings * u * size, size = the sum of the absolute values of the terms of the reference's own sum;
  coordinate    the float32 texel coordinate x = frac(u) * W_l - 0.5 is off by at most `dx` texels PER PIXEL (coord_err below: zero where the
                three operations are exact), and the sample moves by at most dx * the reference's own slope there;
  level         the float32 level is off by at most `dlv` (level64 below) and the sample moves by dlv * |sample(l + 1) - sample(l)|.
All three are continuous across a floor flip (the tap that appears or disappears has weight -> 0): where the reference sits within the
displacement of a cell border or of an integer level, the neighbouring cell's slope / the neighbouring level pair is taken into the maximum,
so NO pixel is excluded anywhere.  K = 4 is the safety factor for log2f / sqrtf being a few ulps off and for fma contraction changing which
roundings happen; it was fixed before the first GPU run."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32 (half an ulp of 1)
K = 4.0                 # safety factor of every bound
TINY = 2.0 ** -126      # one flushed denormal per rounding (float atomics may flush)

# roundings of one fetched value per term of its sum: the tap weight (1 - fx, 1 - fy, their product: 3), the product with the texel and the three
# adds of the bilinear sum (4), the level weight 1 - f and the product with it (2), the add into the output (1)
NR_FETCH = 10
# roundings of one tap weight as texir_tex_taps stores it: 1 - fx, 1 - fy, their product, 1 - f, the product with it
NR_WEIGHT = 5
# a gradient texel summed from n taps: the weight's own roundings, the product with the level weight and with g (the scatter; the gather fuses it), one add per tap
NR_TAP = NR_WEIGHT + 3
# one mip level: 0.25 * (((a + b) + c) + d) -- three adds, each partial sum at most the whole sum a + b + c + d = 4 * `size` (the mean absolute value; the
# product with 0.25 is exact): 3 roundings of `size` per level
NR_MIP = 3
# one fold level: a single fused multiply-add per fine texel
NR_FOLD = 1

SHAPES = [(1, 1, 3, 13), (2, 2, 1, 13), (2, 2, 4, 13), (1, 64, 3, 13), (64, 1, 2, 13), (3, 5, 3, 13), (6, 10, 3, 13), (10, 6, 3, 13),
          (96, 160, 2, 13), (80, 48, 3, 13), (128, 32, 1, 13), (64, 64, 3, 0), (64, 64, 3, 1), (64, 64, 3, 2), (256, 256, 4, 3),
          (1024, 2048, 3, 13), (2048, 1360, 3, 13), (4096, 4096, 1, 13)]
MODES = ("linear", "linear-mipmap-linear")


def shape_id(s):
    return "%dx%dx%d_m%d" % s


def is_pow2(n):
    return n & (n - 1) == 0


# ---- the level structure ---------------------------------------------------------------------------------------------------------------------

def levels_ref(H, W, max_mip_level):
    """number of levels of the chain, level 0 included"""
    n, h, w = 1, H, W
    while n <= max_mip_level and n < 16 and h % 2 == 0 and w % 2 == 0:
        h, w, n = h // 2, w // 2, n + 1
    return n


def level_dims(H, W, levels):
    return [(H >> l, W >> l) for l in range(levels)]


def stack_offsets(H, W, levels):
    """texel offset of every level in the unified stack [level 0 | level 1 | ...] (the keys of texir_tex_taps), and the stack's length"""
    offs, o = [], 0
    for h, w in level_dims(H, W, levels):
        offs.append(o)
        o += h * w
    return offs, o


def rest_offsets(H, W, levels):
    """texel offsets of levels 1.. inside the `rest` buffer (level 0 is the texture itself)"""
    offs, _ = stack_offsets(H, W, levels)
    return [None] + [o - H * W for o in offs[1:]]


# ---- mip chain -------------------------------------------------------------------------------------------------------------------------------

def box2(a, w=(0.25, 0.25, 0.25, 0.25)):
    return w[0] * a[0::2, 0::2] + w[1] * a[0::2, 1::2] + w[2] * a[1::2, 0::2] + w[3] * a[1::2, 1::2]


def mip_chain64(src, n_more, mut_level=None, first=1):
    """n_more further levels below `src` (a float32 level: exact).  -> lists (values, err) per produced level; err = the float32 model's
    error of that level: what the source level's error averages to, plus NR_MIP roundings of the mean absolute value.
    mut_level (mutant): the level with that index (the first produced one has index `first`) is built with weights (.25, .25, .25, .25 + 1e-5)"""
    vals, errs = [], []
    v, e = np.asarray(src, np.float64), np.zeros(np.shape(src))
    for k in range(n_more):
        w = (0.25, 0.25, 0.25, 0.25 + 1e-5) if mut_level == first + k else (0.25,) * 4
        e = box2(e) + NR_MIP * (U * box2(np.abs(v)) + TINY)
        v = box2(v, w)
        vals.append(v)
        errs.append(e)
    return vals, errs


def mip_stack64(tex, levels, mut_level=None):
    """every level in float64 from the float32 level 0 -> (values [levels], err [levels])"""
    vals, errs = mip_chain64(tex, levels - 1, mut_level)
    return [np.asarray(tex, np.float64)] + vals, [np.zeros(np.shape(tex))] + errs


def flat_stack(vals):
    return np.concatenate([v.reshape(-1, v.shape[-1]) for v in vals], 0)


# ---- the rounding model of the coordinates and of the level -------------------------------------------------------------------------------------

def coord_err(uf, frac, n):
    """bound on |x32 - x64| in texels, x = frac(u) * n - 0.5 evaluated in float32 (three operations, each off by at most half an ulp of its result):
      frac  u - floor(u) is exact for u >= 0 and for u <= -1 (the fraction is a multiple of ulp(u) below 1: representable); for -1 < u < 0 the
            result 1 - |u| lies in (0, 1] and rounds by at most 2^-25: n * 2^-25 texels;
      *n    exact when n is a power of two, else at most u * |frac * n|;
      -.5   exact when frac * n >= 1 (the result is no larger and on the same grid), else at most u * |x|.
    Then fx = x - floor(x) is exact for x >= 0 and rounds by at most 2^-25 for -0.5 <= x < 0."""
    x = frac * n - 0.5
    e = np.where((uf < 0) & (uf > -1), n * 2.0 ** -25, 0.0)
    if not is_pow2(n):
        e = e + U * np.abs(frac * n)
    e = e + np.where(frac * n < 1, U * np.abs(x), 0.0)
    return e + np.where(x < 0, 2.0 ** -25, 0.0)


def level64(da, H, W):
    """-> (lv unclamped, dlv): the level in float64 and the bound on the float32 level's distance from it.
    With s = A + B and every input product rounded once (relative u; exact for power-of-two sides):
      dsdx .. dtdy  relative u each (0 for a power-of-two side)           -> squares and products relative 3 u, A, B (sums of positives) relative 4 u
      Cc            may cancel: absolute 4 u (|dsdx dsdy| + |dtdx dtdy|) <= 2 u s =: eC
      l2b           0.5 (A + B): relative 5 u
      A - B         absolute 4 u s + u |A - B| <= 5 u s =: eD
      l2n           0.25 (A - B)^2 + Cc^2: absolute E = 0.25 (2 |A - B| eD + eD^2) + 2 |Cc| eC + eC^2 + 2 u l2n (the squares' own roundings, the add)
      sqrt(l2n)     absolute min(E / sqrt(l2n), sqrt(E)) + u sqrt(l2n) -- the sqrt cannot amplify beyond sqrt(E): no cancellation relative to major,
                    because major >= l2b = s / 2 while sqrt(E) is of order u s where l2n vanishes
      major         absolute eM = 5 u l2b + the above + u major
      lv            0.5 * log2(major): eM / (2 ln 2 major), plus log2f itself: 2 ulps of its result = 2^-22 |log2 major| (times 0.5: exact)
    The clamp, floor and lv - floor(lv) are exact."""
    da = np.asarray(da, np.float64)
    dsdx, dsdy, dtdx, dtdy = da[:, 0] * W, da[:, 1] * W, da[:, 2] * H, da[:, 3] * H
    A, B, Cc = dsdx * dsdx + dtdx * dtdx, dsdy * dsdy + dtdy * dtdy, dsdx * dsdy + dtdx * dtdy
    s = A + B
    l2b, l2n = 0.5 * s, 0.25 * (A - B) ** 2 + Cc * Cc
    major = l2b + np.sqrt(l2n)
    eC, eD = 2 * U * s, 5 * U * s
    E = 0.25 * (2 * np.abs(A - B) * eD + eD * eD) + 2 * np.abs(Cc) * eC + eC * eC + 2 * U * l2n
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sqrt = np.where(l2n > 0, np.minimum(E / np.sqrt(l2n), np.sqrt(E)), np.sqrt(E)) + U * np.sqrt(l2n)
        eM = 5 * U * l2b + e_sqrt + U * major
        lv = 0.5 * np.log2(major)
        dlv = np.where(major > 0, eM / (2 * np.log(2.0) * major) + 2.0 ** -23 * np.abs(2 * lv), 0.0)
    return lv, dlv


# ---- the operator ------------------------------------------------------------------------------------------------------------------------------

class Slot:
    """one mip level a pixel samples (or, a phantom, could sample after a floor flip of the float32 level): per pixel the level, its blend weight,
    the four taps' unified indices and weights, the continuous coordinates and the displacement bounds"""
    pass


def _bilinear64(uf, vf, h, w, mut):
    fu, fv = uf - np.floor(uf), vf - np.floor(vf)
    centre = 0.5 + (1e-3 if mut == "centre" else 0.0)
    x, y = fu * w - centre, fv * h - centre
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    if mut == "clamp_hi":
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    else:
        x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    x0, y0 = x0 % w, y0 % h
    wts = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    if mut == "swap":
        wts[1], wts[2] = wts[2], wts[1]
    idx = [y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1]
    return dict(x=x, y=y, x0=x0, y0=y0, fx=fx, fy=fy, idx=np.stack(idx, 1), w=np.stack(wts, 1), dx=coord_err(uf, fu, w), dy=coord_err(vf, fv, h))


def taps64(H, W, levels, uv, uv_da, mode, mut=None):
    """-> dict: idx [P,8] unified texel indices and w [P,8] weights (first four: floor(level), last four: the next level; a pass with blend weight 0
    keeps its indices with weight 0), lv [P] the unclamped level, dlv [P] its float32 displacement bound, slots: the per-level records (two real ones,
    then the phantoms of a possible floor flip of the level, present only where they can occur).
    mode: 'linear' (level 0 only) or 'linear-mipmap-linear'."""
    uv = np.asarray(uv, np.float64)
    P = uv.shape[0]
    uf, vf = uv[:, 0], uv[:, 1]
    dims = level_dims(H, W, levels)
    offs, _ = stack_offsets(H, W, levels)
    top = levels - 1
    if mode == "linear-mipmap-linear" and levels > 1:
        lv_raw, dlv = level64(uv_da, H, W)
        if mut == "lv_bias":
            lv_raw = lv_raw + 1e-4
        lv = np.clip(lv_raw, 0.0, float(max(top - 1, 0) if mut == "lv_clamp" else top))
        l0 = np.floor(lv).astype(np.int64)
        l1 = np.minimum(l0 + 1, top)
        f = lv - l0
        # a level further than K * dlv outside [0, top] is clamped in float32 as well: no displacement
        m = K * dlv + 2.0 ** -40
        dlv = np.where((lv_raw < -m) | (lv_raw > top + m), 0.0, dlv)
    else:
        lv_raw, dlv = np.full(P, -np.inf), np.zeros(P)
        l0 = l1 = np.zeros(P, np.int64)
        f = np.zeros(P)
        m = np.zeros(P)
    cand = [(l0, 1 - f, np.ones(P, bool)), (l1, f, np.ones(P, bool)),
            (l0 - 1, np.zeros(P), (dlv > 0) & (f <= m) & (l0 >= 1)),                      # the float32 level may fall below floor(level)
            (l1 + 1, np.zeros(P), (dlv > 0) & (1 - f <= m) & (l1 + 1 <= top) & (l1 > l0))]  # ... or reach the level after next
    slots = []
    for lvl, wl, valid in cand:
        s = Slot()
        s.lvl, s.wl, s.valid = np.where(valid, lvl, 0), np.where(valid, wl, 0.0), valid
        s.idx, s.w = np.zeros((P, 4), np.int64), np.zeros((P, 4))
        s.dims = np.ones((P, 2), np.int64)
        for name in ("x", "y", "fx", "fy", "dx", "dy"):
            setattr(s, name, np.zeros(P))
        s.x0, s.y0 = np.zeros(P, np.int64), np.zeros(P, np.int64)
        for l in np.unique(s.lvl[valid]):
            sel = valid & (s.lvl == l)
            h, w = dims[l]
            b = _bilinear64(uf[sel], vf[sel], h, w, mut)
            s.idx[sel], s.w[sel] = b["idx"] + offs[l], b["w"]
            s.dims[sel] = (h, w)
            for name in ("x", "y", "fx", "fy", "dx", "dy", "x0", "y0"):
                getattr(s, name)[sel] = b[name]
        slots.append(s)
    return dict(idx=np.concatenate([slots[0].idx, slots[1].idx], 1),
                w=np.concatenate([slots[0].w * slots[0].wl[:, None], slots[1].w * slots[1].wl[:, None]], 1),
                lv=lv_raw, dlv=dlv, slots=slots, P=P, offs=offs, dims=dims)


def _at(flat, offs_of, dims_of, yy, xx):
    """stack values [P,C] at the (wrapped) texel (yy, xx) of each pixel's level (offs_of [P], dims_of [P,2])"""
    h, w = dims_of[:, 0], dims_of[:, 1]
    return flat[offs_of + (yy % h) * w + (xx % w)]


def forward64(T, flat):
    """fetched values [P,C] of the operator T over the float64 stack `flat` [n_stack,C] -> (values, bound)"""
    out = np.einsum("pk,pkc->pc", T["w"], flat[T["idx"]])
    size = np.einsum("pk,pkc->pc", np.abs(T["w"]), np.abs(flat[T["idx"]]))
    coord = np.zeros_like(out)
    samples = []
    for s in T["slots"]:
        t = flat[s.idx]                                                   # [P,4,C]
        samples.append(np.einsum("pk,pkc->pc", s.w, t))
    for s in T["slots"][:2]:
        # the reference's own slope: the largest horizontal (vertical) difference of neighbouring texels over the cell and -- where the pixel sits within
        # the displacement of a cell border -- over the neighbouring cell the float32 pixel may land in; rows (columns) likewise
        offs_of = s.idx[:, 0] - (s.y0 * s.dims[:, 1] + s.x0)
        mx, my = K * s.dx + 2.0 ** -30, K * s.dy + 2.0 ** -30
        xs = s.x0 + np.where(s.fx <= mx, -1, 0) + np.where(1 - s.fx <= mx, 1, 0)
        ys = s.y0 + np.where(s.fy <= my, -1, 0) + np.where(1 - s.fy <= my, 1, 0)
        g = lambda yy, xx: _at(flat, offs_of, s.dims, yy, xx)
        sx = np.zeros_like(out)
        sy = np.zeros_like(out)
        for yy in (s.y0, s.y0 + 1, ys, ys + 1):
            for xc in (s.x0, xs):
                sx = np.maximum(sx, np.abs(g(yy, xc + 1) - g(yy, xc)))
        for xx in (s.x0, s.x0 + 1, xs, xs + 1):
            for yc in (s.y0, ys):
                sy = np.maximum(sy, np.abs(g(yc + 1, xx) - g(yc, xx)))
        coord += s.wl[:, None] * (s.dx[:, None] * sx + s.dy[:, None] * sy)
    pair = lambda a, b: np.where((T["slots"][a].valid & T["slots"][b].valid)[:, None], np.abs(samples[a] - samples[b]), 0.0)
    level = T["dlv"][:, None] * np.maximum(pair(0, 1), np.maximum(pair(2, 0), pair(1, 3)))
    return out, K * (NR_FETCH * (U * size + TINY) + coord + level)


def weight_bounds(T):
    """per slot the bound on the change of ANY tap weight of that level (every texel's weight is wl * hat(x) * hat(y): Lipschitz 1 in x, y and in
    the level): wl * (dx + dy) + dlv.  [P] per slot, 0 where the slot is absent"""
    return [np.where(s.valid, np.minimum(s.wl + T["dlv"], 1.0) * (s.dx + s.dy) + T["dlv"], 0.0) for s in T["slots"]]


def dense64(T, n_stack):
    """the operator as a dense [P, n_stack] matrix and the entrywise bound of its float32 evaluation (coordinate + level parts: the same value for every
    texel of a level the pixel samples or could sample, zero for every other level; plus the weight's own roundings)"""
    P = T["P"]
    Wm = np.zeros((P, n_stack))
    np.add.at(Wm, (np.arange(P)[:, None], T["idx"]), T["w"])
    B = np.zeros((P, n_stack))
    ends = T["offs"][1:] + [n_stack]
    for s, wb in zip(T["slots"], weight_bounds(T)):
        for l in np.unique(s.lvl[s.valid]):
            sel = np.nonzero(s.valid & (s.lvl == l))[0]
            B[sel, T["offs"][l]:ends[l]] = np.maximum(B[sel, T["offs"][l]:ends[l]], wb[sel, None])
    return Wm, K * (B + NR_WEIGHT * U * np.abs(Wm))


def drop_tail_mask(idx, live):
    """mutant 'gather that drops the last tap of lists whose length is 1 mod 8': True for the taps that survive.  live [P,8]: the taps that are listed at
    all (those of a level with a non-zero blend weight, whatever their own weight); a list = the live taps of one texel in the order of their flat position,
    as a stable sort by texel forms it"""
    flat_idx, live = idx.reshape(-1), np.asarray(live, bool).reshape(-1)
    pos = np.nonzero(live)[0]
    order = pos[np.argsort(flat_idx[pos], kind="stable")]
    keys = flat_idx[order]
    last = np.ones(len(keys), bool)
    last[:-1] = keys[1:] != keys[:-1]
    cnt = np.bincount(keys, minlength=int(flat_idx.max()) + 1 if len(flat_idx) else 1)
    keep = np.ones(flat_idx.shape, bool)
    keep[order[last & (cnt[keys] % 8 == 1)]] = False
    return keep.reshape(idx.shape)


def live_taps(T):
    """[P,8] bool: the taps a tap list holds (the four taps of a level whose blend weight is not zero)"""
    return np.repeat(np.stack([T["slots"][0].wl != 0, T["slots"][1].wl != 0], 1), 4, 1)


def scatter64(T, g, n_stack, mut=None):
    """the transposed operator applied to g [P,C] (float32 values): raw per-level gradient over the unified stack, before any fold
    -> (grad [n_stack,C], err [n_stack,C]): err = the float32 model's error (without K)"""
    g = np.asarray(g, np.float64)
    C = g.shape[1]
    w = T["w"]
    if mut == "drop_tail":
        w = w * drop_tail_mask(T["idx"], live_taps(T))
    grad, size, err = np.zeros((n_stack, C)), np.zeros((n_stack, C)), np.zeros((n_stack, C))
    cnt = np.zeros(n_stack)
    ag = np.abs(g)
    for k in range(8):
        np.add.at(grad, T["idx"][:, k], w[:, k, None] * g)
        np.add.at(size, T["idx"][:, k], np.abs(T["w"][:, k, None]) * ag)
        np.add.at(cnt, T["idx"][:, k], (T["w"][:, k] != 0).astype(np.float64))
    err += (cnt[:, None] + NR_TAP) * (U * size + TINY * (cnt[:, None] > 0))
    # coordinate and level displacement: every tap weight of the slot may change by weight_bounds; so may the weight of the texel next to the cell where
    # the pixel sits within the displacement of the cell border (it is zero in the reference)
    for s, wb in zip(T["slots"], weight_bounds(T)):
        if not s.valid.any() or not (wb > 0).any():
            continue
        sel = np.nonzero(s.valid & (wb > 0))[0]
        contrib = wb[sel, None] * ag[sel]
        offs_of = s.idx[sel, 0] - (s.y0[sel] * s.dims[sel, 1] + s.x0[sel])
        h, w_ = s.dims[sel, 0], s.dims[sel, 1]
        mx, my = K * s.dx[sel] + 2.0 ** -30, K * s.dy[sel] + 2.0 ** -30
        xs = s.x0[sel] + np.where(s.fx[sel] <= mx, -1, 0)
        xe = s.x0[sel] + 1 + np.where(1 - s.fx[sel] <= mx, 1, 0)
        ys = s.y0[sel] + np.where(s.fy[sel] <= my, -1, 0)
        ye = s.y0[sel] + 1 + np.where(1 - s.fy[sel] <= my, 1, 0)
        for dy_ in range(4):
            for dx_ in range(4):
                yy, xx = ys + dy_, xs + dx_
                inside = (yy <= ye) & (xx <= xe)
                if inside.any():
                    np.add.at(err, (offs_of + (yy % h) * w_ + (xx % w_))[inside], contrib[inside])
    return grad, err


def split_levels(flat, H, W, levels):
    offs, n = stack_offsets(H, W, levels)
    ends = offs[1:] + [n]
    return [flat[o:e].reshape(h, w, -1) for o, e, (h, w) in zip(offs, ends, level_dims(H, W, levels))]


def up2(a):
    return a.repeat(2, 0).repeat(2, 1)


def fold64(grads, errs, to_level, mut_level=None):
    """level l-1 += 0.25 * level l (replicated 2x2) from the top down to `to_level` -> (levels, errs): entry to_level holds everything above folded in, the
    entries below it are the raw levels, the entries above it are None.  One fused multiply-add per fine texel and fold level.
    mut_level (mutant): the fold INTO that level reads its coarse level with the fine level's row stride"""
    cur, cur_e = grads[-1], errs[-1]
    for l in range(len(grads) - 1, to_level, -1):
        if mut_level == l - 1:
            hf, wf = grads[l - 1].shape[:2]
            yy, xx = np.meshgrid(np.arange(hf), np.arange(wf), indexing="ij")
            up = cur.reshape(-1, cur.shape[-1])[((yy >> 1) * wf + (xx >> 1)) % (cur.shape[0] * cur.shape[1])]
        else:
            up = up2(cur)
        cur_e = errs[l - 1] + 0.25 * up2(cur_e) + NR_FOLD * (U * (np.abs(grads[l - 1]) + 0.25 * np.abs(up2(cur))) + TINY)
        cur = grads[l - 1] + 0.25 * up
    n_above = len(grads) - 1 - to_level
    return list(grads[:to_level]) + [cur] + [None] * n_above, list(errs[:to_level]) + [cur_e] + [None] * n_above


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------------

RATIOS = {}


def check(got, ref, bound, family, what=""):
    """every element on its own: |got - ref| <= bound (bound already holds K).  Records the worst error / bound of the family and prints it."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (family, what, got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), "%s %s: non-finite values" % (family, what)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    print("error/bound %-10s %-48s %.4f" % (family, what, worst))
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s %s: %d of %d elements outside the bound; worst at %s: got %r, reference %r, bound %.3e (error / bound %.3g)"
                             % (family, what, int((ratio > 1).sum()), ratio.size, i, float(got[i]), float(ref[i]), float(bound[i]), worst))
    return worst


def rejected(got, ref, bound):
    """does check() refuse `got`?  (the mutant tests)"""
    try:
        check(got, ref, bound, "mutant")
    except AssertionError:
        return True
    return False


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------------

F32 = np.float32
SPECIAL = [0.0, 1.0, -1.0, 2.0, 1.0 - 2.0 ** -24, -2.0 ** -30, 0.5]


def make_texture(H, W, C, seed=0):
    return np.random.default_rng([seed, H, W, C]).random((H, W, C), F32)


def lattice(levels_sides, rng, per_level=12):
    """float32 coordinates on the exact lattice of every level: texel centres, edges and quarter texels, the first and last texels always, then a
    random choice; plus the special values"""
    out = list(SPECIAL) + [1e6 + 0.25]
    for n in levels_sides:
        ii = np.unique(np.concatenate([[0, n - 1, n // 2], rng.integers(0, n, per_level)])) if n > per_level else np.arange(n)
        for frac in (0.5, 0.0, 0.25):
            out += list((ii.astype(F32) + F32(frac)) / F32(n))
            out += list((ii[:2].astype(F32) + F32(frac)) / F32(n) - F32(1.0))           # the same lattice one period below zero
        out.append(F32(n) / F32(n))
    return np.asarray(out, F32)


def footprints(H, W, levels, n, rng):
    """[n,4] float32 (du/dX, du/dY, dv/dX, dv/dY), the kinds of the issue dealt round-robin"""
    da = np.zeros((n, 4), np.float64)
    big = max(H, W)
    kinds = 8
    for i in range(n):
        k, a = i % kinds, 10.0 ** rng.uniform(-6, 1)
        if k == 0:
            pass                                                          # zero footprint
        elif k == 1:
            da[i] = a * rng.uniform(0.1, 1.0, 4)                          # log-uniform over [1e-6, 10]
        elif k == 2:
            j = (i // kinds) % (levels + 1)                               # integer levels, the clamp, one past the clamp
            da[i] = (2.0 ** j / W, 0, 0, 2.0 ** j / H)
        elif k == 3:
            da[i] = (a, 0, 0, a / 100)                                    # anisotropic
        elif k == 4:
            b = a * rng.uniform(0.1, 1.0)
            da[i] = (a / W, b / W, b / H, a / H)                          # A == B, Cc != 0
            da[i] *= min(1.0, 10.0 / np.abs(da[i]).max())
        elif k == 5:
            da[i] = a * rng.uniform(-1.0, 1.0, 4)                         # negative components
        elif k == 6:
            da[i] = 10.0 ** rng.uniform(1, 15) / big * rng.uniform(-1.0, 1.0, 4)      # huge: the level clamps at the top (squares stay finite in float32)
        else:
            lvl = rng.uniform(-0.5, levels - 0.5)                         # isotropic, the level uniform over the whole chain
            da[i] = (2.0 ** lvl / W, 0, 0, 2.0 ** lvl / H)
    return da.astype(F32)


def coordinates(H, W, levels, n_random=1500, seed=1):
    """uv [P,2], uv_da [P,4] float32: random pixels in [-1.3, 2.3]^2, then the lattice of every level -- each lattice u with a lattice v and with a
    random v (and the other way round) --; footprints of every kind over all of them"""
    rng = np.random.default_rng([seed, H, W, levels])
    dims = level_dims(H, W, levels)
    lu, lv = lattice([w for _, w in dims], rng), lattice([h for h, _ in dims], rng)
    rnd = lambda n: rng.uniform(-1.3, 2.3, n).astype(F32)
    uv = [np.stack([rnd(n_random), rnd(n_random)], 1),
          np.stack([lu, rng.choice(lv, len(lu))], 1), np.stack([rng.choice(lu, len(lv)), lv], 1),
          np.stack([lu, rnd(len(lu))], 1), np.stack([rnd(len(lv)), lv], 1),
          np.stack(np.meshgrid(np.asarray(SPECIAL, F32), np.asarray(SPECIAL, F32)), -1).reshape(-1, 2)]
    uv = np.ascontiguousarray(np.concatenate(uv, 0), F32)
    return uv, footprints(H, W, levels, len(uv), rng)


def same_uv_pixels(shape, P):
    """P pixels at one uv, footprint between levels 0 and 1: every touched texel's tap list has length P"""
    uv = np.tile(np.array([[0.3712, 0.6291]], F32), (P, 1))
    return uv, np.tile(np.array([[0.7 / shape[1], 0, 0, 0.7 * 2.3 / shape[0]]], F32), (P, 1))


def make_d_out(P, C, seed=2):
    return np.random.default_rng([seed, P, C]).standard_normal((P, C)).astype(F32)


# ---- the mutants of section 3 of the issue ------------------------------------------------------------------------------------------------------
# name -> (keyword arguments of the reference functions, does the mutant change the operator at this shape and mode?)

def _applies_any(H, W, levels, mode):
    return max(H, W) >= 2


def _applies_tri(H, W, levels, mode):
    return mode == "linear-mipmap-linear" and levels >= 2


MUTANTS = {
    "centre": _applies_any,            # texel-centre offset 0.5 -> 0.5 + 1e-3
    "swap": _applies_any,              # w10 and w01 exchanged
    "clamp_hi": _applies_any,          # wrap replaced by clamp on the high edge only
    "lv_bias": _applies_tri,           # level biased by 1e-4
    "lv_clamp": _applies_tri,          # level clamped at levels - 2
    "mip_w": _applies_tri,             # one mip level built with weights (.25, .25, .25, .25 + 1e-5)
    "fold_stride": lambda H, W, levels, mode: _applies_tri(H, W, levels, mode) and H >= 4,   # the fold into level 0 reads level 1 with level 0's row stride
    # gather that drops the last tap of lists whose length is 1 mod 8 (a level one texel wide or high lists every texel an even number of times per pixel: never)
    "drop_tail": lambda H, W, levels, mode: min(H, W) >= 2,
}


class Case:
    """one (shape, mode): seeded inputs, the reference and the bounds of every family.  mut: build the MUTANT's outputs instead (bounds are the
    reference's own and are never taken from a mutant)"""

    def __init__(self, shape, mode, mut=None, n_random=1500, uv=None, da=None, d_out=None, tex=None, base=None):
        H, W, C, mml = shape
        self.shape, self.mode, self.H, self.W, self.C = shape, mode, H, W, C
        self.levels = levels_ref(H, W, mml) if mode == "linear-mipmap-linear" else 1
        if base is not None:                         # (a mutant of `base`: same inputs)
            tex, uv, da, d_out = base.tex, base.uv, base.da, base.d_out
        self.tex = make_texture(H, W, C) if tex is None else tex
        if uv is None:
            uv, da = coordinates(H, W, levels_ref(H, W, mml), n_random)
        self.uv, self.da = uv, da
        self.P = uv.shape[0]
        self.d_out = make_d_out(self.P, C) if d_out is None else d_out
        self.offs, self.n_stack = stack_offsets(H, W, self.levels)
        if base is not None and mut != "mip_w":
            self.stack, self.stack_err, self.flat = base.stack, base.stack_err, base.flat
        else:
            self.stack, self.stack_err = mip_stack64(self.tex, self.levels, self.levels - 1 if mut == "mip_w" else None)
            self.flat = flat_stack(self.stack)
        tap_mut = mut if mut in ("centre", "swap", "clamp_hi", "lv_bias", "lv_clamp") else None
        self.T = base.T if (base is not None and tap_mut is None) else taps64(H, W, self.levels, uv, da, mode, tap_mut)
        self.mut = mut
        self._fwd = None
        self._scat = base._scatter() if (base is not None and mut == "fold_stride") else None
        self._bwd = {}

    def forward(self):
        if self._fwd is None:
            self._fwd = forward64(self.T, self.flat)
        return self._fwd

    def _scatter(self):
        if self._scat is None:
            self._scat = scatter64(self.T, self.d_out, self.n_stack, "drop_tail" if self.mut == "drop_tail" else None)
        return self._scat

    def backward(self, to_level=0):
        """d loss / d stack for d loss / d out = d_out, folded down to `to_level` -> (levels list, bound list), entries as fold64 returns them"""
        if to_level not in self._bwd:
            grad, err = self._scatter()
            sp = lambda a: split_levels(a, self.H, self.W, self.levels)
            gl, el = fold64(sp(grad), sp(err), to_level, 0 if self.mut == "fold_stride" else None)
            self._bwd[to_level] = (gl, [None if e is None else K * e for e in el])
        return self._bwd[to_level]

    def dense(self):
        return dense64(self.T, self.n_stack)
