"""The optimiser kernels of csrc/adam.hip -- adam_kernel, adam_tex_kernel<C>, adam_tex_vec_kernel<C>, adam_tex_vec_batch_kernel<CSET>, adam_tick_kernel --
and grad_add_masked_kernel (csrc/material.hip) against the float64 restatement of tests/adam_cases.py, PER ELEMENT, inside the bound that restatement
derives from the reference alone (first-order running error analysis, K = 2 fixed before the first run).  Every entry point (texir_adam_step, _step_dev,
_step_tex, _step_tex_dev, _step_tex_dev_batch, texir_adam_tick, texir_grad_add_masked) is compared with the REFERENCE, never with another form of the
code; no element is left out.  tests/test_adam_ref_cpu.py shows without a GPU that the same checks pass an op-by-op float32 emulation and reject operator
mutants (eps inside the root, missing bias correction or clamp, a decimal 1 - beta2, a shifted mask bit, a wrong level-2 index, a wrong fold weight).

Direct C-ABI calls.  p, m, v and mip1 (and the tick's state / hyper) sit between canary zones that are checked after every call; g, g1, g2, both masks
and hyper are compared bit for bit afterwards; buffers read under a mask hold NaN at every clear bit; mip1 is prefilled with NaN; no output may be
non-finite.  Shapes: the smallest at which each piece of launch arithmetic can go wrong (ragged last row segment, several segments, mask words that
straddle rows, the row-pair stride of the vector and of the scalar form, TEXIR_ADAM_GRID_Y rounds, the flat kernel's grid-stride round, all four
batched instantiations, a batch that falls back to the scalar launches), see adam_cases.py.

RECORD (one run on an MI355X, 20 passed; test_zz_record prints every figure, lines starting with RECORD).  Worst error / e over the families, per output:
    texir_adam_step / _step_dev     p 0.997 (spread)   m 0.987 (spread)   v 0.982 (spread)
    texir_adam_step_tex / _tex_dev  p 0.987 (spread)   m 0.990 (cancel)   v 0.967 (cancel)   mip1 0.638 (spread)
    texir_adam_step_tex_dev_batch   p 0.992 (spread)   m 0.944 (spread, cancel)   v 0.973 (cancel)   mip1 0.663 (fresh)
    texir_grad_add_masked           g 1.000
    zero-gradient family: v 0.000 everywhere (v' = 0 exactly), p at most 0.807, m at most 0.860
The tick's pairs are the float32 rounding of the exact value or a neighbour on every record; the module adds 3 s to the GPU run (1.0 s inside the tests).
On a CPU, with the float32 chain evaluated op by op in numpy standing in for the kernels and going through the same check functions: worst error / e
0.997 (flat), 0.99 (texture and batched forms); the legitimate two-rounding m * b1 + g * (1 - b1) reaches 1.77 and passes; every mutant exceeds K = 2 in
every family with a non-zero gradient.  K, the bound and the case list were fixed before the run: no tolerance here comes from a GPU run.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import adam_cases as AC

pytestmark = pytest.mark.gpu

CANARY = -7.0e8
PAD = 64                 # elements on either side (256 bytes of float32: the guarded region keeps torch's 16-byte alignment)
SECONDS = [0.0]


@pytest.fixture(autouse=True)
def _timed():
    t0 = time.perf_counter()
    yield
    SECONDS[0] += time.perf_counter() - t0


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from texir_code_amd import _lib
    return _lib


class Guarded:
    """an in-place / output buffer between two canary zones; arr None: prefilled with NaN"""

    def __init__(self, arr=None, shape=None, dtype=np.float32):
        self.shape = tuple(arr.shape if arr is not None else shape)
        self.n = int(np.prod(self.shape))
        self.dtype = dtype
        whole = np.full(self.n + 2 * PAD, CANARY, dtype)
        whole[PAD:PAD + self.n] = np.nan if arr is None else np.asarray(arr, dtype).ravel()
        self.whole = torch.from_numpy(whole).cuda()
        self.ptr = ctypes.c_void_p(self.whole.data_ptr() + PAD * self.whole.element_size())
        assert self.ptr.value % 16 == 0

    def get(self):
        w = self.whole.cpu().numpy()
        assert (w[:PAD] == self.dtype(CANARY)).all() and (w[PAD + self.n:] == self.dtype(CANARY)).all(), "canary overwritten"
        return w[PAD:PAD + self.n].reshape(self.shape).copy()


class Inputs:
    """read-only device buffers, compared bit for bit after the call (None stays a NULL pointer)"""

    def __init__(self, **arrays):
        self.t, self.keep = {}, {}
        for k, a in arrays.items():
            if a is None:
                continue
            raw = np.ascontiguousarray(a).ravel().view(np.uint8)
            buf = np.zeros(max(raw.size, 16), np.uint8)
            buf[:raw.size] = raw
            self.t[k] = torch.from_numpy(buf).cuda()
            self.keep[k] = buf
            assert self.t[k].data_ptr() % 16 == 0

    def ptr(self, k):
        return ctypes.c_void_p(self.t[k].data_ptr()) if k in self.t else None

    def addr(self, k):
        return self.t[k].data_ptr() if k in self.t else None

    def check(self):
        for k, t in self.t.items():
            assert (t.cpu().numpy() == self.keep[k]).all(), "input %s was modified" % k


def _hyper(c):
    return np.array([c.ss, c.bc], np.float32)


class Dev:
    """the device side of one adam_cases.Case"""

    def __init__(self, c):
        self.c = c
        self.p, self.m, self.v = Guarded(c.p), Guarded(c.m), Guarded(c.v)
        self.mip1 = Guarded(shape=(c.H // 2, c.W // 2, c.C)) if (c.H is not None and c.mip) else None
        self.inp = Inputs(g0=c.g0, mask0=c.mask0, g1=c.g1, mask1=c.mask1, g2=c.g2, hyper=_hyper(c))

    def job(self, api):
        c, i = self.c, self.inp
        return api.AdamTexJob(self.p.ptr.value, i.addr("g0"), i.addr("mask0"), i.addr("g1"), i.addr("mask1"), i.addr("g2"), self.m.ptr.value, self.v.ptr.value,
                              self.mip1.ptr.value if self.mip1 else None, c.H, c.W, c.C, i.addr("hyper"),
                              float(c.b1), float(c.b2), float(c.eps), float(c.lo), float(c.hi))

    def result(self):
        torch.cuda.synchronize()
        self.inp.check()
        return {"p": self.p.get(), "m": self.m.get(), "v": self.v.get(), "mip1": self.mip1.get() if self.mip1 else None}


def run(api, c, entry):
    """one call of a single-texture or flat entry point; returns the outputs"""
    L, d = api.lib(), Dev(c)
    i, st = d.inp, api.stream_ptr()
    mip = d.mip1.ptr if d.mip1 else None
    fl = [float(x) for x in (c.b1, c.b2, c.eps)]
    if entry == "texir_adam_step":
        rc = L.texir_adam_step(d.p.ptr, i.ptr("g0"), d.m.ptr, d.v.ptr, c.n, float(c.lr), *fl, c.step, float(c.lo), float(c.hi), st)
    elif entry == "texir_adam_step_dev":
        rc = L.texir_adam_step_dev(d.p.ptr, i.ptr("g0"), d.m.ptr, d.v.ptr, c.n, i.ptr("hyper"), *fl, float(c.lo), float(c.hi), st)
    elif entry == "texir_adam_step_tex":
        assert c.mask1 is None
        rc = L.texir_adam_step_tex(d.p.ptr, i.ptr("g0"), i.ptr("mask0"), i.ptr("g1"), i.ptr("g2"), d.m.ptr, d.v.ptr, mip, c.H, c.W, c.C, float(c.lr), *fl, c.step,
                                   float(c.lo), float(c.hi), st)
    else:
        assert entry == "texir_adam_step_tex_dev" and c.mask1 is None
        rc = L.texir_adam_step_tex_dev(d.p.ptr, i.ptr("g0"), i.ptr("mask0"), i.ptr("g1"), i.ptr("g2"), d.m.ptr, d.v.ptr, mip, c.H, c.W, c.C, i.ptr("hyper"), *fl,
                                       float(c.lo), float(c.hi), st)
    api.check(rc)
    return d.result()


def _extra(entry):
    return 1 if entry in ("texir_adam_step", "texir_adam_step_tex") else 0         # the forms that derive (step_size, bc2_sqrt) from (lr, step) themselves


def _check_tex_group(api, group):
    specs = AC.tex_specs(group)
    assert specs
    for spec in specs:
        c = AC.tex_case(*spec)
        refs = {}
        for entry in ("texir_adam_step_tex", "texir_adam_step_tex_dev"):
            if entry == "texir_adam_step_tex" and c.g1 is None:
                continue                                              # (needs grad_level1)
            x = _extra(entry)
            if x not in refs:
                refs[x] = AC.reference(c, extra_u=x)
            AC.check_outputs(refs[x], run(api, c, entry), tag=(entry, c.family), what="%s %s" % ((c.H, c.W, c.C), c.form))


@pytest.mark.parametrize("entry", ("texir_adam_step", "texir_adam_step_dev"))
def test_flat_kernel(api, entry):
    for spec in AC.flat_specs():
        c = AC.flat_case(*spec)
        got = run(api, c, entry)
        AC.check_outputs(AC.reference(c, extra_u=_extra(entry)), got, tag=(entry, c.family), what="n = %d %s" % (c.n, spec[1]))
        if c.n == 0:
            assert all(got[k].size == 0 for k in "pmv")               # returned OK; the canaries around the empty buffers are intact


@pytest.mark.parametrize("group", ("vector", "scalar", "cross", "settings", "patterns"))
def test_texture_forms(api, monkeypatch, group):
    monkeypatch.delenv("TEXIR_ADAM_SCALAR", raising=False)
    monkeypatch.delenv("TEXIR_ADAM_GRID_Y", raising=False)
    assert api.env_switch("TEXIR_ADAM_SCALAR") == 0 and api.env_switch("TEXIR_ADAM_GRID_Y") == 0
    _check_tex_group(api, group)


def test_texture_forced_scalar_form(api, monkeypatch):
    monkeypatch.delenv("TEXIR_ADAM_GRID_Y", raising=False)
    monkeypatch.setenv("TEXIR_ADAM_SCALAR", "1")
    assert api.env_switch("TEXIR_ADAM_SCALAR") == 1
    _check_tex_group(api, "forced_scalar")


def test_texture_vector_form_with_capped_grid_rows(api, monkeypatch):
    monkeypatch.delenv("TEXIR_ADAM_SCALAR", raising=False)
    monkeypatch.setenv("TEXIR_ADAM_GRID_Y", str(AC.GRID_Y))
    assert api.env_switch("TEXIR_ADAM_GRID_Y") == AC.GRID_Y and api.env_switch("TEXIR_ADAM_SCALAR") == 0
    _check_tex_group(api, "grid_y")


@pytest.mark.parametrize("name", sorted(AC.BATCHES))
def test_batched_step(api, monkeypatch, name):
    monkeypatch.delenv("TEXIR_ADAM_SCALAR", raising=False)
    monkeypatch.delenv("TEXIR_ADAM_GRID_Y", raising=False)
    assert api.env_switch("TEXIR_ADAM_SCALAR") == 0 and api.env_switch("TEXIR_ADAM_GRID_Y") == 0
    assert len(AC.BATCHES[name]) <= api.MAX_BATCH
    for variant in (0, 1):
        cases = AC.batch_cases(name, variant)
        devs = [Dev(c) for c in cases]
        api.batch_call("texir_adam_step_tex_dev_batch", [d.job(api) for d in devs])
        for k, (c, d) in enumerate(zip(cases, devs)):
            AC.check_outputs(AC.reference(c), d.result(), tag=("texir_adam_step_tex_dev_batch", c.family), what="%s job %d %s %s" % (name, k, (c.H, c.W, c.C), c.form))


def test_adam_tick(api):
    L = api.lib()
    for n in AC.TICK_N:
        for seed in (range(12) if 0 < n < 12 else (0, 5)):
            for mask in AC.tick_masks(n):
                st0, hy0 = AC.tick_state(n, seed)
                state, hyper = Guarded(st0, dtype=np.float64), Guarded(hy0)
                for _ in range(2):                                    # two consecutive ticks on the same buffers
                    api.check(L.texir_adam_tick(state.ptr, hyper.ptr, n, mask, api.stream_ptr()))
                    torch.cuda.synchronize()
                    st1, hy1 = state.get(), hyper.get()
                    AC.check_tick(st0, hy0, mask, st1, hy1)
                    st0, hy0 = st1, hy1


def test_grad_add_masked(api):
    L = api.lib()
    shapes = [(n, C) for n in (1, 31, 32, 33, 1296) for C in (1, 2, 3, 4)] + [(350001, 3)]
    k = 0
    for (n, C) in shapes:
        for pat in AC.MASK_PATTERNS:
            if not AC.pattern_fits(pat, n) or (n > 2000 and pat not in ("half", "last")):
                continue
            k += 1
            c = AC.grad_add_case(n, C, pat, AC.FAMILIES[k % len(AC.FAMILIES)], 8000 + k)
            g, inp = Guarded(c.g), Inputs(g0=c.g0, mask=c.mask)
            api.check(L.texir_grad_add_masked(g.ptr, inp.ptr("g0"), inp.ptr("mask"), n, C, api.stream_ptr()))
            torch.cuda.synchronize()
            inp.check()
            AC.check_grad_add(c, g.get(), tag=("texir_grad_add_masked", c.family))
    g = Guarded(np.zeros((0, 3), np.float32))
    api.check(L.texir_grad_add_masked(g.ptr, None, None, 0, 3, api.stream_ptr()))       # n = 0: OK, nothing read or written
    torch.cuda.synchronize()
    g.get()


def test_zz_record():
    """prints the record the module docstring keeps (run last)"""
    for (entry, fam) in sorted(AC.RATIOS):
        print("RECORD ratio %-30s %-9s %s" % (entry, fam, " ".join("%s %.3f" % kv for kv in sorted(AC.RATIOS[(entry, fam)].items()))))
    print("RECORD seconds %.1f" % SECONDS[0])
