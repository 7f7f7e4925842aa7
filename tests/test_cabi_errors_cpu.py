"""CPU: the refusals of the material-side entry points of libtexir_hip.so -- return code and message text, byte for byte, as recorded from the library
before its two C ABIs (capi.hip and the batched block of material.hip) became one.  Every call below is refused by an argument check that returns
before the first HIP call, so nothing is dereferenced and no device is needed; the pointers are dummies."""
import ctypes as C

import pytest

INVALID = -1                # TEXIR_ERR_INVALID
D = 8                       # a dummy non-null pointer


@pytest.fixture(scope="module")
def L():
    import os
    from texir_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def refused(L, name, args, msg, getter="texir_last_error"):
    rc = getattr(L, name)(*args)
    got = getattr(L, getter)().decode()
    assert (rc, got) == (INVALID, "%s: %s" % (name, msg)), (name, args)
    return got


def fetch_job(**kw):
    from texir_code_amd._lib import TexFetchJob
    a = dict(tex=D, mips_rest=D, H=8, W=8, C=3, levels=2, build_from=-1, filter_mode=1, uv=D, uv_da=D, P=4, out=D)
    a.update(kw)
    return TexFetchJob(**a)


def gather_job(**kw):
    from texir_code_amd._lib import TexGatherJob
    a = dict(d_tex=D, grad_rest=D, H=8, W=8, C=3, levels=2, seg_key=D, seg_start=D, seg_count=D, n_seg=1, pix=D, weights=D, d_out=D, filter_mode=1,
             defer_last_fold=0, rest_mask=None, d_out2=None)
    a.update(kw)
    return TexGatherJob(**a)


def adam_job(**kw):
    from texir_code_amd._lib import AdamTexJob
    a = dict(param=D, grad=D, grad_mask=None, grad_level1=D, level1_mask=None, grad_level2=None, exp_avg=D, exp_avg_sq=D, mip_level1=None, H=8, W=8, C=3,
             hyper=D, beta1=0.9, beta2=0.999, eps=1e-8, clamp_lo=0.0, clamp_hi=1.0)
    a.update(kw)
    return AdamTexJob(**a)


# the single-texture calls' argument lists from the job structures of their batched forms (include/texir_hip.h)
def fetch_args(q):
    return (q.tex, q.mips_rest, q.H, q.W, q.C, q.levels, q.uv, q.uv_da, q.filter_mode, q.P, q.out, None)


def gather_args(q):
    return (q.d_tex, q.grad_rest, q.H, q.W, q.C, q.levels, q.seg_key, q.seg_start, q.seg_count, q.n_seg, q.pix, q.weights, q.d_out, q.filter_mode,
            q.defer_last_fold, None)


def adam_args(q):
    return (q.param, q.grad, q.grad_mask, q.grad_level1, q.grad_level2, q.exp_avg, q.exp_avg_sq, q.mip_level1, q.H, q.W, q.C, q.hyper, q.beta1, q.beta2,
            q.eps, q.clamp_lo, q.clamp_hi, None)


def batch_refused(L, name, job, msg, n=1):
    arr = (type(job) * 1)(job)
    return refused(L, name, (arr, n, None), msg, getter="texir_batch_last_error")


def both_refused(L, single, args_of, job, msg):
    """the same bad job through the single-texture call and through its batched form: the same words, apart from the function's name and `job 0: `"""
    a = refused(L, single, args_of(job), msg)
    b = batch_refused(L, single + "_batch", job, "job 0: " + msg)
    assert b.replace(single + "_batch: job 0: ", single + ": ") == a


BAD_TEX = "bad texture H=8 W=8 C=5 levels=2"
NO_LEVELS = "5 mip levels not available for 8x8"


def test_mip_build(L):
    ok = dict(tex=D, rest=D, H=8, W=8, C=3, levels=2, from_level=0)
    def call(msg, **kw):
        refused(L, "texir_mip_build", tuple({**ok, **kw}.values()) + (None,), msg)
    call("null argument", tex=None)
    call("null argument", rest=None)
    call("from_level must be 0 or 1", from_level=2)
    call("from_level must be 0 or 1", from_level=-1)
    call(BAD_TEX, C=5)
    call("bad texture H=0 W=8 C=3 levels=2", H=0)
    call("bad texture H=8 W=8 C=3 levels=17", levels=17)
    call("bad texture H=8 W=8 C=3 levels=0", levels=0)
    call(NO_LEVELS, levels=5)
    call("2 mip levels not available for 7x8", H=7)


def test_fetch_forward_single_and_batched(L):
    for bad in (dict(tex=None), dict(uv=None), dict(out=None), dict(uv_da=None), dict(mips_rest=None)):
        both_refused(L, "texir_tex_fetch_forward", fetch_args, fetch_job(**bad), "null argument")
    both_refused(L, "texir_tex_fetch_forward", fetch_args, fetch_job(C=5), BAD_TEX)
    both_refused(L, "texir_tex_fetch_forward", fetch_args, fetch_job(levels=5), NO_LEVELS)
    # the one rule whose words differ: the batched form names its third field
    for bad in (dict(filter_mode=2), dict(filter_mode=-1, uv_da=None, mips_rest=None), dict(P=-1)):
        refused(L, "texir_tex_fetch_forward", fetch_args(fetch_job(**bad)), "bad filter_mode/P")
        batch_refused(L, "texir_tex_fetch_forward_batch", fetch_job(**bad), "job 0: bad filter_mode/P/build_from")
    for bf in (-2, 2):
        batch_refused(L, "texir_tex_fetch_forward_batch", fetch_job(build_from=bf), "job 0: bad filter_mode/P/build_from")
    # the single call demands uv / out even at P = 0; the batched one takes such a job and goes on to the next rule
    for bad in (dict(uv=None), dict(out=None), dict(uv_da=None)):
        refused(L, "texir_tex_fetch_forward", fetch_args(fetch_job(P=0, C=5, **bad)), "null argument")
        batch_refused(L, "texir_tex_fetch_forward_batch", fetch_job(P=0, C=5, **bad), "job 0: " + BAD_TEX)
    batch_refused(L, "texir_tex_fetch_forward_batch", fetch_job(filter_mode=0, build_from=0, mips_rest=None), "job 0: a build needs mips_rest")
    # the job that is refused names itself
    arr = (type(fetch_job()) * 2)(fetch_job(P=0), fetch_job(C=5))
    refused(L, "texir_tex_fetch_forward_batch", (arr, 2, None), "job 1: " + BAD_TEX, getter="texir_batch_last_error")


def test_fetch_backward_and_taps(L):
    def bwd(q):
        return (q.tex, q.mips_rest, q.H, q.W, q.C, q.levels, q.uv, q.uv_da, q.filter_mode, q.P, q.out, None)
    def deferred(q):
        return (q.tex, q.mips_rest, q.H, q.W, q.C, q.levels, q.uv, q.uv_da, q.P, q.out, None)
    def taps(q):
        return (q.H, q.W, q.C, q.levels, q.uv, q.uv_da, q.filter_mode, q.P, q.tex, q.out, None)
    for bad in (dict(tex=None), dict(uv=None), dict(out=None), dict(uv_da=None), dict(mips_rest=None)):
        refused(L, "texir_tex_fetch_backward", bwd(fetch_job(**bad)), "null argument")
        refused(L, "texir_tex_fetch_backward_deferred", deferred(fetch_job(**bad)), "null argument")
    refused(L, "texir_tex_fetch_backward_deferred", deferred(fetch_job(filter_mode=0, uv_da=None)), "null argument")
    for bad in (dict(tex=None), dict(uv=None), dict(out=None), dict(uv_da=None)):            # (keys, uv, weights, uv_da)
        refused(L, "texir_tex_taps", taps(fetch_job(**bad)), "null argument")
    for bad in (dict(filter_mode=2), dict(P=-1)):
        refused(L, "texir_tex_fetch_backward", bwd(fetch_job(**bad)), "bad filter_mode/P")
        refused(L, "texir_tex_taps", taps(fetch_job(**bad)), "bad filter_mode/P")
    for bad in (dict(P=-1), dict(levels=1)):
        refused(L, "texir_tex_fetch_backward_deferred", deferred(fetch_job(**bad)), "needs P >= 0 and at least two mip levels")
    for name, args in (("texir_tex_fetch_backward", bwd), ("texir_tex_fetch_backward_deferred", deferred), ("texir_tex_taps", taps)):
        refused(L, name, args(fetch_job(C=5)), BAD_TEX)
        refused(L, name, args(fetch_job(levels=5)), NO_LEVELS)


def test_gather_backward_single_and_batched(L):
    fn = "texir_tex_gather_backward"
    for bad in (dict(d_tex=None), dict(d_out=None), dict(seg_key=None), dict(seg_start=None), dict(seg_count=None), dict(pix=None), dict(weights=None),
                dict(grad_rest=None)):
        both_refused(L, fn, gather_args, gather_job(**bad), "null argument")
    # d_tex may be NULL with a deferred fold: the job passes the null rule and is refused by the next one that applies
    both_refused(L, fn, gather_args, gather_job(d_tex=None, defer_last_fold=1, C=5), BAD_TEX)
    # ... and the lists may be NULL when there are none
    both_refused(L, fn, gather_args, gather_job(n_seg=0, seg_key=None, seg_start=None, seg_count=None, pix=None, weights=None, C=5), BAD_TEX)
    big = dict(H=32, W=32, levels=4)
    for bad in (dict(filter_mode=2), dict(filter_mode=-1, grad_rest=None), dict(n_seg=-1), dict(defer_last_fold=-1), dict(defer_last_fold=3),
                dict(defer_last_fold=1, filter_mode=0), dict(defer_last_fold=1, levels=1), dict(defer_last_fold=2, H=32, W=32, levels=3),
                dict(defer_last_fold=2, **{**big, "H": 34}), dict(defer_last_fold=2, **{**big, "W": 34})):
        both_refused(L, fn, gather_args, gather_job(**bad), "bad filter_mode/n_seg/defer_last_fold")
    both_refused(L, fn, gather_args, gather_job(C=5), BAD_TEX)
    both_refused(L, fn, gather_args, gather_job(levels=5), NO_LEVELS)
    both_refused(L, fn, gather_args, gather_job(defer_last_fold=2, **{**big, "levels": 7}), "7 mip levels not available for 32x32")
    # rules of the batched form alone
    for f in (0, 1):
        batch_refused(L, fn + "_batch", gather_job(rest_mask=D, defer_last_fold=f), "job 0: rest_mask needs defer_last_fold = 2")
    batch_refused(L, fn + "_batch", gather_job(rest_mask=D, d_out2=D, defer_last_fold=2, C=5, **big), "job 0: bad texture H=32 W=32 C=5 levels=4")


def test_gather_backward_batch_per_level_rules(L, monkeypatch):
    from texir_code_amd import _lib
    monkeypatch.setenv("TEXIR_MIP_PER_LEVEL", "1")
    assert _lib.env_switch("TEXIR_MIP_PER_LEVEL") == 1
    fn = "texir_tex_gather_backward_batch"
    batch_refused(L, fn, gather_job(d_out2=D), "job 0: d_out2 is not available with TEXIR_MIP_PER_LEVEL=1")
    batch_refused(L, fn, gather_job(d_out2=D, rest_mask=D), "job 0: d_out2 is not available with TEXIR_MIP_PER_LEVEL=1")
    batch_refused(L, fn, gather_job(rest_mask=D, defer_last_fold=1), "job 0: rest_mask needs defer_last_fold = 2")
    batch_refused(L, fn, gather_job(rest_mask=D, defer_last_fold=2, H=32, W=32, levels=4),
                  "job 0: rest_mask is not available with TEXIR_MIP_PER_LEVEL=1 (the per-level folds read a cleared stack)")


def test_adam_tex_dev_single_and_batched(L):
    fn = "texir_adam_step_tex_dev"
    for bad in (dict(param=None), dict(grad_level1=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(hyper=None)):
        both_refused(L, fn, adam_args, adam_job(**bad), "null argument")
    # grad_level1 may be NULL beside a level-2 gradient
    both_refused(L, fn, adam_args, adam_job(grad_level1=None, grad_level2=D, C=5), "bad H/W/C")
    for bad in (dict(H=3), dict(H=0), dict(W=1), dict(W=6, H=7), dict(C=0), dict(C=5)):
        both_refused(L, fn, adam_args, adam_job(**bad), "bad H/W/C")
    for bad in (dict(H=6), dict(W=10)):
        both_refused(L, fn, adam_args, adam_job(grad_level2=D, **bad), "a level-2 gradient needs H and W divisible by 4")
    batch_refused(L, fn + "_batch", adam_job(level1_mask=D), "job 0: level1_mask needs grad_level2")
    arr = (type(adam_job()) * 2)(adam_job(), adam_job(H=3))        # (job 0 is complete: the checks walk all jobs before anything is launched)
    refused(L, fn + "_batch", (arr, 2, None), "job 1: bad H/W/C", getter="texir_batch_last_error")


def test_adam_host_step_forms(L):
    def tex(q, step=1):
        return (q.param, q.grad, q.grad_mask, q.grad_level1, q.grad_level2, q.exp_avg, q.exp_avg_sq, q.mip_level1, q.H, q.W, q.C, 1e-3, q.beta1, q.beta2,
                q.eps, step, q.clamp_lo, q.clamp_hi, None)
    fn = "texir_adam_step_tex"
    for bad in (dict(param=None), dict(grad_level1=None), dict(grad_level1=None, grad_level2=D), dict(exp_avg=None), dict(exp_avg_sq=None)):
        refused(L, fn, tex(adam_job(**bad)), "null argument")
    for bad in (dict(H=3), dict(W=0), dict(C=5)):
        refused(L, fn, tex(adam_job(**bad)), "bad H/W/C/step")
    refused(L, fn, tex(adam_job(), step=0), "bad H/W/C/step")
    refused(L, fn, tex(adam_job(grad_level2=D, H=6)), "a level-2 gradient needs H and W divisible by 4")
    ok = dict(param=D, grad=D, exp_avg=D, exp_avg_sq=D, n=4, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, lo=0.0, hi=1.0)
    for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
        refused(L, "texir_adam_step", tuple({**ok, k: None}.values()) + (None,), "null argument")
    refused(L, "texir_adam_step", tuple({**ok, "n": -1}.values()) + (None,), "bad n/step")
    refused(L, "texir_adam_step", tuple({**ok, "step": 0}.values()) + (None,), "bad n/step")
    refused(L, "texir_adam_tick", (None, D, 1, 1, None), "null argument")
    refused(L, "texir_adam_tick", (D, None, 1, 1, None), "null argument")
    refused(L, "texir_adam_tick", (D, D, 65, 1, None), "0..64 records per call (got 65)")
    refused(L, "texir_adam_tick", (D, D, -1, 1, None), "0..64 records per call (got -1)")


def test_grad_add_masked_and_job_counts(L):
    B = "texir_batch_last_error"
    refused(L, "texir_grad_add_masked", (None, None, None, 4, 9, None), "bad size n_texels=4 C=9", getter=B)
    refused(L, "texir_grad_add_masked", (D, D, D, -1, 3, None), "bad size n_texels=-1 C=3", getter=B)
    refused(L, "texir_grad_add_masked", (D, D, D, 4, 0, None), "bad size n_texels=4 C=0", getter=B)
    for args in ((None, D, D), (D, None, D), (D, D, None)):
        refused(L, "texir_grad_add_masked", args + (4, 3, None), "null argument", getter=B)
    for name, job in (("texir_tex_fetch_forward_batch", fetch_job()), ("texir_tex_gather_backward_batch", gather_job()),
                      ("texir_adam_step_tex_dev_batch", adam_job())):
        arr = (type(job) * 1)(job)
        refused(L, name, (arr, 5, None), "0..4 jobs (got 5)", getter=B)
        refused(L, name, (arr, -1, None), "0..4 jobs (got -1)", getter=B)
        refused(L, name, (None, 1, None), "0..4 jobs (got 1)", getter=B)
        assert getattr(L, name)(None, 0, None) == 0                     # no jobs: nothing to do, nothing launched


def test_one_error_text_for_both_getters(L):
    """the library has one error string: after a refused batched call texir_last_error() holds that call's message too (before the two C ABIs were
    joined it kept whatever the last single-texture call had left)"""
    refused(L, "texir_mip_build", (None, None, 8, 8, 3, 2, 0, None), "null argument")
    msg = batch_refused(L, "texir_adam_step_tex_dev_batch", adam_job(H=3), "job 0: bad H/W/C")
    assert L.texir_last_error().decode() == msg == L.texir_batch_last_error().decode()
