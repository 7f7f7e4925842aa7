"""The float64 texture restatement of tests/texture_cases.py and its checker, tested without a GPU:
  * a legitimate float32 implementation -- oracle/ref_torch.texture and its autograd on the CPU -- passes check() at every shape of the GPU matrix;
  * every mutant of section 3 of the issue (texture_cases.MUTANTS) is rejected by the same check() at every power-of-two shape of the matrix and at
    every other shape with sides up to 256 where it changes the operator.
So the bound is neither too tight for float32 nor blind to a wrong tap, weight, level, mip or fold."""
import functools
import os

import numpy as np
import pytest
import torch

import texture_cases as TC


@pytest.fixture(autouse=True)
def _bounded_intraop_threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)), prev)))
    yield
    torch.set_num_threads(prev)


N_RANDOM = 600


@functools.lru_cache(maxsize=None)
def _small_case(shape, mode):
    return TC.Case(shape, mode, n_random=N_RANDOM)


def ref_case(shape, mode):
    """(the large shapes are rebuilt per use: their float64 stacks are too big to keep)"""
    if shape[0] * shape[1] > 300000:
        return TC.Case(shape, mode, n_random=N_RANDOM)
    return _small_case(shape, mode)


def test_level_structure():
    assert TC.levels_ref(3, 5, 13) == 1 and TC.levels_ref(6, 10, 13) == 2 and TC.levels_ref(80, 48, 13) == 5 and TC.levels_ref(128, 32, 13) == 6
    assert TC.levels_ref(64, 64, 0) == 1 and TC.levels_ref(64, 64, 2) == 3 and TC.levels_ref(4096, 4096, 13) == 13 and TC.levels_ref(1 << 20, 1 << 20, 99) == 16
    offs, n = TC.stack_offsets(6, 10, 2)
    assert offs == [0, 60] and n == 75 and TC.rest_offsets(6, 10, 2) == [None, 0]


def test_operator_is_a_partition_of_unity_and_hits_texel_centres():
    """rows of the operator sum to 1; a pixel at the centre of texel (i, j) of level 0 with a zero footprint reads exactly that texel"""
    H, W, C = 6, 10, 3
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    uv = np.stack([(jj.reshape(-1) + 0.5) / W, (ii.reshape(-1) + 0.5) / H], 1).astype(np.float64)
    T = TC.taps64(H, W, 2, uv, np.zeros((H * W, 4)), "linear-mipmap-linear")
    Wm, _ = TC.dense64(T, 75)
    assert np.allclose(Wm.sum(1), 1.0, atol=1e-12)
    assert np.allclose(Wm[:, :60], np.eye(60), atol=1e-9) and np.abs(Wm[:, 60:]).max() == 0
    # footprint of exactly two texels: level 1 alone, and the four taps of the centre of a level-0 texel there weigh 9/16, 3/16, 3/16, 1/16
    da = np.tile(np.array([[2.0 / W, 0, 0, 2.0 / H]]), (H * W, 1))
    T = TC.taps64(H, W, 2, uv, da, "linear-mipmap-linear")
    Wm, _ = TC.dense64(T, 75)
    assert np.abs(Wm[:, :60]).max() == 0 and np.allclose(np.sort(Wm[0, 60:])[-4:], [1 / 16, 3 / 16, 3 / 16, 9 / 16])


def test_check_itself():
    ref, bound = np.array([1.0, 2.0]), np.array([1e-6, 0.0])
    assert TC.check(np.array([1.0 + 5e-7, 2.0]), ref, bound, "self") == pytest.approx(0.5)
    assert TC.rejected(np.array([1.0, 2.0 + 1e-12]), ref, bound)              # a zero bound demands the exact value
    assert TC.rejected(np.array([1.0 + 2e-6, 2.0]), ref, bound)
    assert TC.rejected(np.array([np.nan, 2.0]), ref, bound)


def test_drop_tail_mask():
    idx = np.array([[3, 3, 5, 7, 7, 7, 7, 7]] * 2)
    w = np.ones((2, 8))
    w[1, 2] = 0.0                                # texel 5: one live tap (dropped); texel 3: four; texel 7: ten
    keep = TC.drop_tail_mask(idx, w != 0)
    assert keep.sum() == 15 and not keep[0, 2]
    idx = np.zeros((9, 8), np.int64) + np.arange(8)     # eight texels with nine taps each: the last pixel's taps go
    keep = TC.drop_tail_mask(idx, np.ones((9, 8), bool))
    assert keep[:8].all() and not keep[8].any()


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.shape_id)
def test_float32_torch_restatement_is_inside_the_bound(shape):
    """oracle/ref_torch.texture (float32, CPU) and its autograd: mip chain, forward and complete gradient, both filter modes"""
    from oracle import ref_torch as RT
    H, W, C, mml = shape
    for mode in TC.MODES:
        c = ref_case(shape, mode)
        tex = torch.from_numpy(c.tex).clone().requires_grad_(True)
        with torch.no_grad():
            stack = RT.mip_stack(tex, mml) if mode != "linear" else [tex]
        assert len(stack) == c.levels
        for l in range(1, c.levels):
            TC.check(stack[l].numpy(), c.stack[l], TC.K * c.stack_err[l], "ref-mip", "%s level %d" % (TC.shape_id(shape), l))
        out = RT.texture(tex, torch.from_numpy(c.uv), torch.from_numpy(c.da), mode, mml)
        ref, bound = c.forward()
        TC.check(out.detach().numpy(), ref, bound, "ref-fwd", "%s %s" % (TC.shape_id(shape), mode))
        (out * torch.from_numpy(c.d_out)).sum().backward()
        gl, bl = c.backward(0)
        # (autograd folds with a product and an add per level instead of one fused multiply-add, and its index backward adds tap by tap: both inside K)
        TC.check(tex.grad.numpy(), gl[0], bl[0], "ref-bwd", "%s %s" % (TC.shape_id(shape), mode))


def _eligible(shape):
    H, W = shape[:2]
    return (TC.is_pow2(H) and TC.is_pow2(W)) or max(H, W) <= 256


def _mutant_rejected(ref, mut):
    """is the mutant's output refused in at least one family (mip chain, dense operator, forward, complete gradient)?  The bounds are the reference's"""
    m = TC.Case(ref.shape, ref.mode, mut=mut, base=ref)
    if mut == "mip_w":
        return any(TC.rejected(m.stack[l], ref.stack[l], TC.K * ref.stack_err[l]) for l in range(1, ref.levels))
    if mut in ("fold_stride", "drop_tail"):
        return TC.rejected(m.backward(0)[0][0], ref.backward(0)[0][0], ref.backward(0)[1][0])
    if ref.n_stack <= 2000:
        Wm, B = ref.dense()
        if not TC.rejected(m.dense()[0], Wm, B):
            return False                      # (the small shapes must see the mutant in the operator itself, not only in the fetched values)
    return TC.rejected(m.forward()[0], ref.forward()[0], ref.forward()[1])


@pytest.mark.parametrize("mut", sorted(TC.MUTANTS))
def test_mutant_is_rejected(mut):
    expected, seen = [], []
    for shape in TC.SHAPES:
        if not _eligible(shape):
            continue
        for mode in TC.MODES:
            levels = TC.levels_ref(shape[0], shape[1], shape[3]) if mode != "linear" else 1
            if not TC.MUTANTS[mut](shape[0], shape[1], levels, mode):
                continue
            expected.append((TC.shape_id(shape), mode))
            ref = ref_case(shape, mode)
            if mut == "drop_tail" and shape[0] * shape[1] <= 4:
                # (four texels that every pixel taps: one list per texel, thousands of taps long, whose length is 1 mod 8 by chance only and whose last tap
                # is below the rounding of the sum.  The case that exposes the mutant there: nine pixels, zero footprint -- four lists of nine)
                ref = TC.Case(shape, mode, uv=ref.uv[:9], da=np.zeros((9, 4), np.float32))
            if _mutant_rejected(ref, mut):
                seen.append(expected[-1])
    print("mutant %s rejected at: %s" % (mut, ", ".join("%s/%s" % s for s in seen)))
    assert expected, "mutant %s changes the operator nowhere in the matrix" % mut
    assert seen == expected, "mutant %s NOT rejected at %s" % (mut, [s for s in expected if s not in seen])


@pytest.mark.parametrize("P", [1, 7, 8, 9, 15, 16, 17, 64, 1001])
def test_dropped_last_tap_is_rejected_on_lists_of_one_length(P):
    """all P pixels at one uv: the mutant changes the gradient exactly where P is 1 mod 8"""
    shape = (64, 64, 3, 13)
    uv, da = TC.same_uv_pixels(shape, P)
    for mode in TC.MODES:
        ref = TC.Case(shape, mode, uv=uv, da=da)
        m = TC.Case(shape, mode, mut="drop_tail", base=ref)
        assert TC.rejected(m.backward(0)[0][0], ref.backward(0)[0][0], ref.backward(0)[1][0]) == (P % 8 == 1), (P, mode)
