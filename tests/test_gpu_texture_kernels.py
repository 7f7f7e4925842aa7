"""The texture path of csrc/material.hip (the file holds nothing else: the G-buffer is csrc/gbuffer.hip, the optimiser csrc/adam.hip) -- mip build, level selection, wrap-bilinear taps, fetch, the three backward forms and the gradient folds --
against the float64 restatement of tests/texture_cases.py, element by element inside a bound derived from a float32 rounding model (K = 4, fixed
before the first run; see texture_cases for the derivation).  No pixel and no texel is excluded from any comparison.  Every form of the code
(pyramid and TEXIR_MIP_PER_LEVEL=1, scatter / deferred / gather with fold_to_level 0, 1, 2, single and batched launches) is compared with the
REFERENCE, never with another form.  tests/test_texture_ref_cpu.py shows, without a GPU, that the same check() passes a legitimate float32
implementation and rejects every mutant of the operator.

Non-finite coordinates are not run here.  Read from the code and from the gfx950 ISA of tex_taps_kernel / tex_fetch_kernel: after
`u - floorf(u)` a coordinate is in [0, 1] or NaN (inf - inf), so floor(x) lies in [-1, W - 1] or is NaN, and the conversion is emitted as
v_cvt_i32_f32, which saturates and turns NaN into 0: x0 = 0, x1 = 1 (0 for a one-texel side) -- every index stays in range, the weights
(and that pixel's output or its four level-0 gradient texels) are NaN.  The level goes through v_max_f32(0, lv), v_min_f32(.., levels - 1): a NaN
level becomes 0, +inf the top level.  So no out-of-range address is possible and no guard was added; what a NaN pixel returns stays unspecified.

Worst error / bound seen on the MI355X per family (1.0 = the bound):
  mip 0.24   taps 0.25   fwd 0.25   bwd-scatter 0.25   bwd-deferred 0.25   bwd-gather 0.25   public-fwd 0.22   public-bwd 0.18
(the worst cases are lattice pixels whose float32 coordinate rounds by exactly the half ulp the model allows: error = bound / K).  The module adds about
40 s to the GPU run, most of it the float64 reference of the 2^20 + 777-pixel and the 1.5 M-pixel cases.
"""
import functools
import os

import numpy as np
import pytest
import torch

import texture_cases as TC

pytestmark = pytest.mark.gpu

TRI = "linear-mipmap-linear"


@pytest.fixture(autouse=True)
def _bounded_intraop_threads():
    """the float64 restatement runs numpy / torch CPU ops on up to 1.5 M pixels: keep torch to the CPUs this process may use (at most 16), and hand
    back the previous setting after each test"""
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)), prev)))
    yield
    torch.set_num_threads(prev)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- direct calls of the C-ABI -----------------------------------------------------------------------------------------------------------------

class Gpu:
    """the device side of one texture_cases.Case"""

    def __init__(self, case):
        from texir_code_amd import _lib
        self._lib, self.L, self.c = _lib, _lib.lib(), case
        self.H, self.W, self.C, self.levels = case.H, case.W, case.C, case.levels
        self.mode = 1 if case.mode == TRI else 0
        self.tex, self.uv, self.da, self.g = _dev(case.tex), _dev(case.uv), _dev(case.da), _dev(case.d_out)
        self.n_rest = int(self.L.texir_mip_elems(self.H, self.W, self.C, self.levels))
        assert int(self.L.texir_mip_levels(self.H, self.W, case.shape[3])) == TC.levels_ref(self.H, self.W, case.shape[3])
        assert self.n_rest == max(1, (case.n_stack - self.H * self.W) * self.C)
        self.dims = (self.H, self.W, self.C, self.levels)

    def call(self, name, *args):
        p = self._lib.ptr
        self._lib.check(getattr(self.L, name)(*[p(a) if isinstance(a, torch.Tensor) else a for a in args], self._lib.stream_ptr()))
        torch.cuda.synchronize()

    def rest_levels(self, rest):
        """levels 1.. of a `rest` buffer as float64 [h,w,C] arrays (index 0: None)"""
        r = rest.cpu().numpy().astype(np.float64)
        out = [None]
        for l in range(1, self.levels):
            h, w = self.H >> l, self.W >> l
            o = TC.rest_offsets(self.H, self.W, self.levels)[l] * self.C
            out.append(r[o:o + h * w * self.C].reshape(h, w, self.C))
        return out

    def mip_build(self, from_level=0, rest=None):
        if rest is None:
            rest = torch.full((self.n_rest,), float("nan"), device="cuda")
        self.call("texir_mip_build", self.tex, rest, *self.dims, from_level)
        return rest

    def taps(self):
        keys = torch.full((self.c.P * 8,), -7, device="cuda", dtype=torch.int64)
        w = torch.full((self.c.P * 8,), float("nan"), device="cuda")
        self.call("texir_tex_taps", *self.dims, self.uv, self.da, self.mode, self.c.P, keys, w)
        return keys.cpu().numpy().reshape(-1, 8), w.cpu().numpy().reshape(-1, 8)

    def forward(self, rest):
        out = torch.full((self.c.P, self.C), float("nan"), device="cuda")
        self.call("texir_tex_fetch_forward", self.tex, rest, *self.dims, self.uv, self.da, self.mode, self.c.P, out)
        return out.cpu().numpy()

    def backward(self, form, fold, lists=None, g=None):
        """form 'scatter' (fold 0: texir_tex_fetch_backward, 1: ..._deferred) or 'gather' (fold 0 / 1 / 2) -> (d_tex [H,W,C], rest levels) float64"""
        g = self.g if g is None else g
        d_tex = torch.zeros(self.H, self.W, self.C, device="cuda")
        rest = torch.zeros(self.n_rest, device="cuda")
        if form == "scatter" and fold == 0:
            self.call("texir_tex_fetch_backward", d_tex, rest, *self.dims, self.uv, self.da, self.mode, self.c.P, g)
        elif form == "scatter":
            self.call("texir_tex_fetch_backward_deferred", d_tex, rest, *self.dims, self.uv, self.da, self.c.P, g)
        else:
            seg_key, starts, counts, pix, wts = lists
            self.call("texir_tex_gather_backward", d_tex, rest, *self.dims, seg_key, starts, counts, int(seg_key.numel()), pix, wts, g, self.mode, fold)
        return d_tex.cpu().numpy().astype(np.float64), self.rest_levels(rest)


def tap_lists(keys, w, mode):
    """the caller's part of the gather backward (include/texir_hip.h): taps sorted by key (stable), segments per touched texel"""
    k = keys.copy()
    if mode == 0:
        k[:, 4:] = -1
    k = k.reshape(-1)
    order = np.argsort(k, kind="stable")
    order = order[np.searchsorted(k[order], 0):]
    seg_key, starts, counts = np.unique(k[order], return_index=True, return_counts=True)
    return (_dev(seg_key.astype(np.int64)), _dev(starts.astype(np.int32)), _dev(counts.astype(np.int32)), _dev((order // 8).astype(np.int32)),
            _dev(w.reshape(-1)[order].astype(np.float32)))


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------------------

def check_mip(gpu, rest, what, first=1, src=None):
    """levels first.. of `rest` against the float64 chain (from level 0, or from the float32 level first - 1 given as src)"""
    c = gpu.c
    if src is None:
        vals, errs = c.stack[1:], c.stack_err[1:]
    else:
        vals, errs = TC.mip_chain64(src, c.levels - first, first=first)
    got = gpu.rest_levels(rest)
    for k, l in enumerate(range(first, c.levels)):
        TC.check(got[l], vals[k], TC.K * errs[k], "mip", "%s level %d" % (what, l))


def check_taps(gpu, keys, w, what):
    c = gpu.c
    live = keys >= 0
    assert ((keys == -1) | (live & (keys < c.n_stack))).all(), "%s: tap key out of range" % what
    assert np.isfinite(w).all() and (w[~live] == 0).all()
    # a pass is skipped exactly when its blend weight is zero: the four keys of a pass go together
    assert (live[:, :4].all(1) | ~live[:, :4].any(1)).all() and (live[:, 4:].all(1) | ~live[:, 4:].any(1)).all()
    if c.n_stack <= 2000:
        # the operator itself: indices and weights entry by entry, immune to floor flips
        Wg = np.zeros((c.P, c.n_stack))
        rows = np.broadcast_to(np.arange(c.P)[:, None], keys.shape)
        np.add.at(Wg, (rows[live], keys[live]), w[live].astype(np.float64))
        Wm, B = c.dense()
        TC.check(Wg, Wm, B, "taps", what + " dense operator")
    # the listed operator applied to the float64 stack
    ref, bound = c.forward()
    out = np.einsum("pk,pkc->pc", np.where(live, w, 0).astype(np.float64), c.flat[np.where(live, keys, 0)])
    TC.check(out, ref, bound, "taps", what + " applied")


def check_bwd(gpu, d_tex, rest, fold, family, what):
    """the parked levels as they are, then the COMPLETE level-0 gradient after the remaining folds in float64"""
    c = gpu.c
    gl, bl = c.backward(fold)
    got = [d_tex] + rest[1:fold + 1]
    for l in range(fold + 1):
        TC.check(got[l], gl[l], bl[l], family, "%s fold_to %d level %d" % (what, fold, l))
    cur = got[fold]
    for l in range(fold - 1, -1, -1):
        cur = got[l] + 0.25 * TC.up2(cur)
    if fold:
        g0, b0 = c.backward(0)
        TC.check(cur, g0[0], b0[0], family, "%s fold_to %d complete" % (what, fold))


def folds_of(c):
    if c.mode != TRI or c.levels < 2:
        return [0]
    return [0, 1] + ([2] if (c.levels >= 4 and c.H % 4 == 0 and c.W % 4 == 0) else [])


def run_all(c, what, forms=("mip", "taps", "fwd", "scatter", "gather")):
    """every entry point of the path on one case"""
    gpu = Gpu(c)
    rest = gpu.mip_build() if c.levels > 1 else torch.zeros(1, device="cuda")
    if c.levels > 1 and "mip" in forms:
        check_mip(gpu, rest, what)
        if c.levels > 2:
            # from_level 1: level 1 is the caller's (the fused optimiser writes it): any float32 values
            h, w = c.H >> 1, c.W >> 1
            l1 = np.random.default_rng(5).random((h, w, c.C), np.float32)
            r1 = torch.full((gpu.n_rest,), float("nan"), device="cuda")
            r1[:l1.size] = _dev(l1.reshape(-1))
            gpu.mip_build(1, r1)
            assert np.array_equal(gpu.rest_levels(r1)[1], l1.astype(np.float64)), "from_level 1 rewrote level 1"
            check_mip(gpu, r1, what + " from_level 1", first=2, src=l1)
    keys = w = None
    if "taps" in forms or "gather" in forms:
        keys, w = gpu.taps()
    if "taps" in forms:
        check_taps(gpu, keys, w, what)
    if "fwd" in forms:
        ref, bound = c.forward()
        TC.check(gpu.forward(rest), ref, bound, "fwd", what)
    lists = tap_lists(keys, w, gpu.mode) if "gather" in forms else None
    for fold in folds_of(c):
        if "scatter" in forms and fold <= 1:
            d_tex, r = gpu.backward("scatter", fold)
            check_bwd(gpu, d_tex, r, fold, "bwd-scatter" if fold == 0 else "bwd-deferred", what)
        if "gather" in forms:
            d_tex, r = gpu.backward("gather", fold, lists)
            check_bwd(gpu, d_tex, r, fold, "bwd-gather", what)
    return gpu, lists


# ---- the case matrix ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def matrix_case(shape, mode):
    """(one reference per shape and mode: the pyramid and the per-level run share it)"""
    return TC.Case(shape, mode)


MATRIX = [(s, m, pl) for s in TC.SHAPES for m in TC.MODES for pl in (0, 1)]


@pytest.mark.parametrize("shape,mode,per_level", MATRIX, ids=["%s-%s-%s" % (TC.shape_id(s), m, "per_level" if pl else "pyramid") for s, m, pl in MATRIX])
def test_matrix(tx, monkeypatch, shape, mode, per_level):
    if per_level:
        monkeypatch.setenv("TEXIR_MIP_PER_LEVEL", "1")
    else:
        monkeypatch.delenv("TEXIR_MIP_PER_LEVEL", raising=False)
    from texir_code_amd import _lib
    assert _lib.env_switch("TEXIR_MIP_PER_LEVEL") == per_level
    run_all(matrix_case(shape, mode), "%s %s %s" % (TC.shape_id(shape), mode, "per-level" if per_level else "pyramid"))


def test_check_tex_limits_are_refused(tx):
    from texir_code_amd import _lib
    L = _lib.lib()
    t, r, uv, da, out = (torch.zeros(n, device="cuda") for n in (64 * 64 * 4, 64 * 64 * 4, 2, 4, 4))
    keys = torch.zeros(8, device="cuda", dtype=torch.int64)
    p = _lib.ptr
    for H, W, C, levels in [(64, 64, 0, 1), (64, 64, 5, 1), (64, 64, 3, 0), (64, 64, 3, 17), (64, 64, 3, 8), (6, 10, 3, 3), (3, 5, 3, 2), (0, 64, 3, 1)]:
        for rc in (L.texir_mip_build(p(t), p(r), H, W, C, levels, 0, _lib.stream_ptr()),
                   L.texir_tex_fetch_forward(p(t), p(r), H, W, C, levels, p(uv), p(da), 1, 1, p(out), _lib.stream_ptr()),
                   L.texir_tex_fetch_backward(p(t), p(r), H, W, C, levels, p(uv), p(da), 1, 1, p(out), _lib.stream_ptr()),
                   L.texir_tex_taps(H, W, C, levels, p(uv), p(da), 1, 1, p(keys), p(out), _lib.stream_ptr())):
            with pytest.raises(_lib.TexirError):
                _lib.check(rc)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0 and float(r.abs().sum()) == 0        # refused, not run
    _lib.check(L.texir_mip_build(p(t), p(r), 64, 64, 3, 7, 0, _lib.stream_ptr()))


# ---- directed cases ----------------------------------------------------------------------------------------------------------------------------------

def random_case(shape, mode, P, seed=11, **kw):
    H, W, C, mml = shape
    rng = np.random.default_rng([seed, P])
    uv = rng.uniform(-1.3, 2.3, (P, 2)).astype(np.float32)
    return TC.Case(shape, mode, uv=uv, da=TC.footprints(H, W, TC.levels_ref(H, W, mml), P, rng), **kw)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 2 ** 20 + 777])
def test_pixel_counts_around_a_block_and_beyond_the_grid(tx, P):
    """the grid-stride loops of the fetch, scatter and taps kernels (at most 4096 blocks x 256 threads) wrap at 2^20 + 777 pixels"""
    for mode in TC.MODES:
        run_all(random_case((64, 64, 3, 13), mode, P), "64x64x3 P=%d %s" % (P, mode), forms=("taps", "fwd", "scatter", "gather"))


@pytest.mark.parametrize("P", [1, 7, 8, 9, 15, 16, 17, 64, 1001])
def test_gather_lists_of_one_length(tx, P):
    """all P pixels at one uv: every touched texel's list has length P (rounds of eight taps, the clamped tail re-read, the look-ahead loads)"""
    shape = (64, 64, 3, 13)
    uv, da = TC.same_uv_pixels(shape, P)
    for mode in TC.MODES:
        c = TC.Case(shape, mode, uv=uv, da=da)
        gpu, lists = run_all(c, "one uv P=%d %s" % (P, mode), forms=("gather",))
        assert (lists[2].cpu().numpy() == P).all() and lists[0].numel() == (4 if mode == "linear" else 8)


def test_gather_four_very_long_lists(tx):
    for mode in TC.MODES:
        c = random_case((2, 2, 3, 13), mode, 20000)
        gpu, lists = run_all(c, "2x2x3 P=20000 %s" % mode, forms=("taps", "fwd", "scatter", "gather"))
        assert int(lists[2].max()) >= 4000


def test_gather_more_segments_than_the_grid(tx):
    """2048x1360x3 with 1.5 M random pixels touches more than 2^20 texels: the gather's segment loop wraps"""
    c = random_case((2048, 1360, 3, 13), TRI, 1500000)
    gpu, lists = run_all(c, "2048x1360x3 P=1.5M", forms=("fwd", "gather"))
    assert lists[0].numel() > 2 ** 20


def test_special_output_gradients(tx):
    """d_out with exact zeros in whole pixels and in single channels (the scatter skips g == 0), with -0.0, and with magnitudes from 1e-30 to 1e30 in one
    launch (400 pixels: no float32 sum of the reference's `size` overflows)"""
    shape, P = (96, 160, 2, 13), 400
    rng = np.random.default_rng(21)
    g = rng.standard_normal((P, 2)) * 10.0 ** rng.uniform(-30, 30, (P, 1))
    g[::5] = 0.0
    g[1::7, 0] = 0.0
    g[2::9, 1] = -0.0
    g[3::11] = -0.0
    for mode in TC.MODES:
        run_all(random_case(shape, mode, P, d_out=g.astype(np.float32)), "special d_out %s" % mode, forms=("scatter", "gather"))


# ---- the public path ---------------------------------------------------------------------------------------------------------------------------------

def _bits(mask, n):
    return ((mask.view(-1, 1).to(torch.int64) >> torch.arange(32, device=mask.device)) & 1).bool().reshape(-1)[:n].cpu().numpy()


def complete_gradient(p):
    """the gradient FusedAdam.step is about to apply to p, reassembled in float64 from the parts step() reads: p.grad (dense) or the never-cleared level-0
    buffer under its bit mask, the parked level-1 stack (under the view's tap mask, or not read at all when no tap touches level 1) and the parked level-2
    stack.  Everything outside a mask was pre-filled with 1e30 by the test: a read outside the mask shows"""
    H, W, C = p.shape
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    g1 = getattr(p, "_texir_grad_l1", None)
    if g1 is None:
        return f64(p.grad)
    g = np.zeros((H, W, C)) if p.grad is None else f64(p.grad)
    if getattr(p, "_texir_l0_sparse", False) and getattr(p, "_texir_l0_mask", None) is not None:
        bits = _bits(p._texir_l0_mask, H * W).reshape(H, W)
        g[bits] += f64(p._texir_g0)[bits]
    g2 = getattr(p, "_texir_grad_l2", None)
    l1 = f64(g1).reshape(H // 2, W // 2, C)
    if g2 is not None and getattr(p, "_texir_l1_zero", False):
        l1 = np.zeros_like(l1)
    elif g2 is not None and getattr(g1, "_texir_mask", None) is not None:
        l1 = np.where(_bits(g1._texir_mask, (H // 2) * (W // 2)).reshape(H // 2, W // 2, 1), l1, 0.0)
    if g2 is not None:
        l1 = l1 + 0.25 * TC.up2(f64(g2).reshape(H // 4, W // 4, C))
    return g + 0.25 * TC.up2(l1)


def _poison_never_cleared(p):
    """1e30 into the buffers the masked backward never clears: the level-0 buffer and the parameter's gradient stack (arena span or own buffer)"""
    if getattr(p, "_texir_g0", None) is not None:
        p._texir_g0.fill_(1e30)
    if getattr(p, "_texir_arena", None) is not None:
        lo, hi = p._texir_arena_span
        p._texir_arena["buf"][lo:hi].fill_(1e30)
        p._texir_arena["clean"].discard(id(p))
    if getattr(p, "_texir_grest", None) is not None:
        p._texir_grest.fill_(1e30)


PUBLIC = [(96, 160, 2, 13), (80, 48, 3, 13), (128, 32, 1, 13)]


@pytest.mark.parametrize("use_cache", [False, True], ids=["cache_none", "cache_dict"])
@pytest.mark.parametrize("param", [False, True], ids=["tensor", "fused_adam"])
def test_public_texture_and_texture_batch(tx, monkeypatch, param, use_cache):
    """texture() and texture_batch() (two and three textures, fanout 2 on one of them) on plain tensors and on nn.Parameters under
    FusedAdam(fuse_mip_fold=True) with default switches: forward values and, after backward(), the complete gradient"""
    for k in ("TEXIR_MIP_PER_LEVEL", "TEXIR_DEFER_LEVELS", "TEXIR_ADAM_SCALAR"):
        monkeypatch.delenv(k, raising=False)
    from texir_code_amd.optim import FusedAdam
    from texir_code_amd.texture import texture, texture_batch
    mode = TRI
    cases = [TC.Case(s, mode) for s in PUBLIC]
    P = min(c.P for c in cases)
    # (one set of coordinates for the batch: those of the first shape; every texture gets its own reference over them)
    uv, da = cases[0].uv[:P], cases[0].da[:P]
    cases = [TC.Case(s, mode, uv=uv, da=da) for s in PUBLIC]
    uv_d, da_d = _dev(uv), _dev(da)

    def make():
        ts = [_dev(c.tex) for c in cases]
        if not param:
            return [t.requires_grad_(True) for t in ts], None
        ps = [torch.nn.Parameter(t) for t in ts]
        return ps, FusedAdam(ps, lr=1e-3, fuse_mip_fold=True)

    def verify(cs, ts, outs, grads_out, what):
        """outs: per texture the list of its hand-outs; grads_out: the gradient sent into each hand-out"""
        for c, os_ in zip(cs, outs):
            ref, bound = c.forward()
            for o in os_:
                TC.check(o.detach().cpu().numpy(), ref, bound, "public-fwd", "%s %s" % (what, TC.shape_id(c.shape)))
        for t in ts:
            _poison_never_cleared(t)
        torch.autograd.backward([o for os_ in outs for o in os_], [g for gs in grads_out for g in gs])
        torch.cuda.synchronize()
        for c, t, gs in zip(cs, ts, grads_out):
            # (two consumers: their gradients are added in float32 -- by the gather or by autograd -- before anything else: the same float either way)
            total = gs[0] if len(gs) == 1 else gs[0] + gs[1]
            cc = TC.Case(c.shape, mode, uv=uv, da=da, d_out=total.cpu().numpy())
            g0, b0 = cc.backward(0)
            TC.check(complete_gradient(t), g0[0], b0[0], "public-bwd", "%s %s" % (what, TC.shape_id(c.shape)))

    def reset(ts, opt):
        if opt is not None:
            opt.zero_grad()
        for t in ts:
            t.grad = None

    rng = np.random.default_rng(31)
    mk_g = lambda c: _dev(rng.standard_normal((P, c.C)).astype(np.float32))
    passes = 2 if use_cache else 1     # (the second pass reuses the view's tap lists and the never-cleared buffers, now full of 1e30 outside the masks)
    # texture(): one texture at a time
    ts, opt = make()
    caches = [({} if use_cache else None) for _ in cases]
    for rep in range(passes):
        reset(ts, opt)
        outs = [[texture(t, uv_d, da_d, mode, 13, cache=ch)] for t, ch in zip(ts, caches)]
        verify(cases, ts, outs, [[mk_g(c)] for c in cases], "texture() pass %d" % rep)
    # texture_batch(): two textures, then three with fanout 2 on the second
    for n, fan in ((2, None), (3, [1, 2, 1])):
        ts, opt = make()
        cache = {} if use_cache else None
        for rep in range(passes):
            reset(ts, opt)
            res = texture_batch(ts[:n], uv_d, da_d, mode, 13, cache=cache, fanout=fan)
            outs = [list(r) if isinstance(r, tuple) else [r] for r in res]
            verify(cases[:n], ts[:n], outs, [[mk_g(c) for _ in os_] for c, os_ in zip(cases[:n], outs)], "texture_batch(%d) pass %d" % (n, rep))
