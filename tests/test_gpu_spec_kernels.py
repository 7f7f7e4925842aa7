"""The GGX specular sample chain of csrc/kernels.hip -- spec_sample, spec_kernel<BWD, WIDTH, DW>, spec_bwd_ws_kernel, gen_dir_kernel and the
sampling helpers of device_common.h -- against the float64 restatement of tests/spec_cases.py, PER SAMPLE and per pixel, inside the bound that
restatement derives for each sample from the reference alone (running error analysis by autograd, K = 4 fixed before the first run; kink variants as
described there).  Every entry point is compared with the REFERENCE, never with another form of the code, and no aggregate norm is used.  The only
samples without a comparison are those with more than 4 uncertain kinks (at most 0.1 % of a case; a per-pixel sum that contains one is not compared
either).  tests/test_spec_ref_cpu.py shows without a GPU that the same checks pass legitimate float32 implementations, reject every operator mutant and
that every case of the matrix respects the caps.

Direct C-ABI calls with lighting given (ls_given = 1, scene NULL: pure arithmetic, no tracer); outputs prefilled with NaN between canaries, inputs
compared bit for bit afterwards.  Per-sample weights w are observed through one-hot lighting (pixel p repeated S times, copy i lit at sample i only,
irr = 0), which also shows a non-finite weight (0 * inf = NaN); dw is read from dw_ws directly.

Not in scope: the traced path (ls_given = 0) stays under the aggregate tests of test_gpu_parity.py: which triangle a ray hits is discontinuous in the
reflected direction l, and l, which only the tracer consumes, cannot be observed through ls_given = 1.  l is checked on the CPU side only
(test_spec_ref_cpu.py: float32 restatement against the float64 one and the golden's l).

No case of the matrix has a non-finite reference value (asserted in test_spec_ref_cpu.py), so no kernel output may be non-finite anywhere.

RECORD (worst error / bound per family and output on the MI355X, shares of multi-variant / left-out / accepted-by-another-variant samples, seconds the
module adds to the GPU run): NOT MEASURED.  No run of this module on an MI355X has been recorded yet; test_zz_record prints every figure of the
record at the end of a run (lines starting with RECORD) so that they can be entered here.  What has been measured, on a CPU only, with the float32
chain evaluated op by op in torch standing in for the kernels and going through the same run_case(): worst error / bound 0.11 for w and 0.11 for dw in
family A (0.09 in B, D, E, F), multi-variant samples 1.2 - 1.9 % in A, 100 % / 61 - 67 % in the r <= 0.02 / [0.02, 0.06] parts of B, none left out, at
most 0.07 % accepted by a variant other than the base one; the float64 references of the specular cases (2.0 M samples) take 73 s on 8 CPU threads, those of
generate_dir were not timed (the texture module's 40 s is not met: the P = 1037 cases at S = 256 and S = 1000 alone are 1.3 M samples of the hooked restatement).
"""
import os

import numpy as np
import pytest
import torch

import spec_cases as SC

pytestmark = pytest.mark.gpu

CANARY = -7.0e8
PAD = 64


@pytest.fixture(autouse=True)
def _bounded_intraop_threads():
    """the float64 restatement runs torch CPU autograd passes on up to 1e6 samples: keep torch to the CPUs this process may use (at most 16), and
    hand back the previous setting after each test"""
    prev = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)), prev)))
    yield
    torch.set_num_threads(prev)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


class Out:
    """an output buffer prefilled with NaN between two canary zones"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.whole = torch.full((self.n + 2 * PAD,), CANARY, device="cuda")
        self.t = self.whole[PAD:PAD + self.n]
        self.t.fill_(float("nan"))

    def get(self):
        w = self.whole.cpu().numpy()
        assert (w[:PAD] == np.float32(CANARY)).all() and (w[PAD + self.n:] == np.float32(CANARY)).all(), "canary overwritten"
        return w[PAD:PAD + self.n].reshape(self.shape).astype(np.float64)


class Gpu:
    """the device side of one spec_cases.Case"""

    def __init__(self, c, L=None):
        from texir_code_amd import _lib
        self._lib, self.lib, self.c = _lib, _lib.lib(), c
        self.P, self.S = c.P, c.S
        self.inp = {k: _dev(getattr(c, k)) for k in ("normal", "albedo", "rough", "points", "irr", "cam", "shift", "d_rgb")}
        self.inp["L"] = _dev(c.L if L is None else L)
        self.keep = {k: v.clone() for k, v in self.inp.items()}

    def call(self, name, *args):
        p = self._lib.ptr
        self._lib.check(getattr(self.lib, name)(*[p(a) if isinstance(a, torch.Tensor) else a for a in args], self._lib.stream_ptr()))
        torch.cuda.synchronize()
        for k, v in self.inp.items():
            assert torch.equal(v.view(torch.int32), self.keep[k].view(torch.int32)), "%s: input %s was modified" % (name, k)

    def forward(self, train=False, inp=None, P=None):
        i = dict(self.inp, **(inp or {}))
        P = self.P if P is None else P
        rgb = Out(P, 3)
        head = (None, i["normal"], i["albedo"], i["rough"], i["points"], i["irr"], i["cam"], i["shift"], P, self.S, float(self.c.ceps), 1, rgb.t, i["L"])
        if train:
            dw = Out(P, self.S)
            self.call("texir_spec_forward_train", *head, dw.t)
            return rgb.get(), dw.get()
        self.call("texir_spec_forward", *head)
        return rgb.get()

    def backward(self, dw=None, need_a=True, need_r=True):
        """texir_spec_backward, or texir_spec_backward_ws on the given dw [P,S] -> (d_albedo | None, d_rough | None)"""
        i = self.inp
        da, dr = Out(self.P, 3), Out(self.P)
        pa, pr = (da.t if need_a else None), (dr.t if need_r else None)
        if dw is None:
            self.call("texir_spec_backward", i["normal"], i["rough"], i["points"], i["irr"], i["cam"], i["shift"], i["L"], i["d_rgb"], self.P, self.S,
                      float(self.c.ceps), pa, pr)
        else:
            self.call("texir_spec_backward_ws", i["irr"], i["L"], dw, i["d_rgb"], self.P, self.S, pa, pr)
        a, r = da.get(), dr.get()
        if not need_a:
            assert np.isnan(a).all(), "d_albedo = NULL: the unused buffer was written"
        if not need_r:
            assert np.isnan(r).all(), "d_rough = NULL: the unused buffer was written"
        return (a if need_a else None), (r if need_r else None)

    def weights(self):
        """per-sample w [P,S] through one-hot lighting: pixel p repeated S times, copy i lit at sample i only, irr = 0 -> rgb[p,i] = w_i / S"""
        c, P, S = self.c, self.P, self.S
        rep = lambda k: self.inp[k].repeat_interleave(S, 0).contiguous()
        L = torch.zeros(P * S, S, 3, device="cuda")
        L[torch.arange(P * S, device="cuda"), torch.arange(S, device="cuda").repeat(P)] = 1.0
        inp = {k: rep(k) for k in ("normal", "albedo", "rough", "points", "shift")}
        inp["irr"], inp["L"] = torch.zeros(P * S, 3, device="cuda"), L
        rgb = self.forward(inp=inp, P=P * S)
        assert np.isfinite(rgb).all(), "%s: non-finite weight" % c.name
        assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 0] == rgb[:, 2]).all()
        return rgb[:, 0] * S


def can_onehot(c):
    return c.P * c.S * c.S * 3 <= 1e7


def run_case(c, fam, forced_lpp=0, nulls=True):
    """every entry point on one case, each against the reference"""
    ref = c.ref()
    assert ref.left.mean() <= SC.CAP_LEFT_OUT
    cap = SC.CAP_NONBASE
    g = Gpu(c)
    what = c.name
    # forward, evaluation form and training form
    c.check_rgb(g.forward(), fam + "-rgb", what + " forward", forced_lpp)
    rgb, dw = g.forward(train=True)
    c.check_rgb(rgb, fam + "-rgb", what + " forward_train", forced_lpp)
    SC.check_deriv(dw.reshape(-1), ref, "dw", fam + "-dw", what + " dw_ws", named=c.named, cap=cap)
    if can_onehot(c):
        w = g.weights()
        SC.check_value(w, ref, "w", fam + "-w", what + " one-hot w", extra=SC.K * SC.U * np.abs(w)[None], named=c.named, cap=cap)
    # backward that recomputes the chain
    da_ref, da_b = c.d_albedo()
    da, dr = g.backward()
    SC.check_exact(da, da_ref, da_b, fam + "-dalb", what + " backward d_albedo")
    c.check_drough(dr, fam + "-drough", what + " backward d_rough", forced_lpp)
    # backward on kept derivatives, fed the reference's own float32-rounded dw
    dw32 = ref.val["dw"][0].astype(np.float32).reshape(c.P, c.S)
    assert np.isfinite(dw32).all()
    exact = SC.exact_ref(dw32)
    d_dw = _dev(dw32)
    da, dr = g.backward(dw=d_dw)
    SC.check_exact(da, da_ref, da_b, fam + "-dalb", what + " backward_ws d_albedo")
    c.check_drough(dr, fam + "-drough-ws", what + " backward_ws d_rough", forced_lpp, ref=exact)
    if nulls:
        for d in (None, d_dw):
            nm = "backward" if d is None else "backward_ws"
            da, _ = g.backward(dw=d, need_r=False)
            SC.check_exact(da, da_ref, da_b, fam + "-dalb", what + " %s d_rough=NULL" % nm)
            _, dr = g.backward(dw=d, need_a=False)
            if d is None:
                c.check_drough(dr, fam + "-drough", what + " backward d_albedo=NULL", forced_lpp)
            else:
                c.check_drough(dr, fam + "-drough-ws", what + " backward_ws d_albedo=NULL", forced_lpp, ref=exact)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SC.S_LIST)
def test_spec_shapes(S):
    """family A at every lane assignment: S lanes per pixel, one partial pass, several passes with a partial last one; P around the pixels per wave"""
    for c in SC.shape_cases(S):
        run_case(c, "A", nulls=c.P != 1037)


@pytest.mark.parametrize("S,P", SC.GRID_CAP_SHAPES)
def test_spec_grid_stride_round(monkeypatch, S, P):
    """TEXIR_SPEC_GRID_CAP = 2: two blocks of 4 waves walk P pixels in three full rounds and a partial one"""
    monkeypatch.setenv("TEXIR_SPEC_GRID_CAP", "2")
    from texir_code_amd import _lib
    assert _lib.env_switch("TEXIR_SPEC_GRID_CAP") == 2
    ppb = 4 * (64 // SC.lanes_per_pixel(S))
    assert 3 * 2 * ppb < P < 4 * 2 * ppb
    run_case(SC.grid_cap_case(S, P), "A-gridcap")


@pytest.mark.parametrize("lpp,S", SC.LPP_SHAPES)
def test_spec_forced_lanes_per_pixel(monkeypatch, lpp, S):
    """TEXIR_SPEC_LPP: fewer lanes and more passes per pixel, below and above a whole number of waves"""
    monkeypatch.setenv("TEXIR_SPEC_LPP", str(lpp))
    from texir_code_amd import _lib
    assert _lib.env_switch("TEXIR_SPEC_LPP") == lpp
    for c in SC.lpp_cases(lpp, S):
        run_case(c, "A-lpp", forced_lpp=lpp, nulls=False)


# ---- input families --------------------------------------------------------------------------------------------------------------------------------

_FAMILY = SC.family_cases()


@pytest.mark.parametrize("c", _FAMILY, ids=[c.name for c in _FAMILY])
def test_spec_families(c):
    run_case(c, c.family)


# ---- scene.spec_render, autograd end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train_form", [True, False])
def test_spec_render_autograd(tx, train_form):
    c = SC.autograd_case()
    prev = tx._TRAIN_FORM[0]
    tx._TRAIN_FORM[0] = train_form
    try:
        alb, r = _dev(c.albedo).requires_grad_(True), _dev(c.rough).requires_grad_(True)
        rgb = tx.spec_render(None, _dev(c.normal), alb, r, _dev(c.points), _dev(c.irr), _dev(c.cam), _dev(c.shift), c.S, clamp_eps=c.ceps, lighting=_dev(c.L))
        (rgb * _dev(c.d_rgb)).sum().backward()
    finally:
        tx._TRAIN_FORM[0] = prev
    fam = "A-autograd"
    c.check_rgb(rgb.detach().cpu().numpy(), fam + "-rgb", "form %d" % train_form)
    da_ref, da_b = c.d_albedo()
    SC.check_exact(alb.grad.cpu().numpy(), da_ref, da_b, fam + "-dalb", "form %d" % train_form)
    c.check_drough(r.grad.cpu().numpy(), fam + "-drough", "form %d" % train_form)


# ---- generate_dir --------------------------------------------------------------------------------------------------------------------------------------

MODE_ID = {"uniform": 0, "cosine": 1, "importance": 2}


def gen_dir_inputs(b, seed):
    rng = np.random.default_rng([seed, b])
    n = np.concatenate([SC.frame_normals(), SC.unit_normals(max(1, b), rng)], 0)
    n = n[rng.permutation(len(n))[:b]] if b < len(n) else np.concatenate([n, SC.unit_normals(b, rng)], 0)[:b]
    r = rng.uniform(0.0, 1.0, b).astype(np.float32)
    r[::7] = (0.0, 0.01, 1.0, 0.8)[seed % 4]
    sh = rng.random((b, 2), np.float32)
    sh[::5] = 0.0
    sh[1::11] = 1.0
    return np.ascontiguousarray(n, np.float32), r, sh


def run_gen_dir(mode, b, N, seed=0):
    from texir_code_amd import _lib
    n, r, sh = gen_dir_inputs(b, seed + N)
    ref = SC.reference(SC.sample_inputs(n, r, None, None, sh, N), mode=mode, names=("d0", "d1", "d2"))
    assert ref.left.mean() <= SC.CAP_LEFT_OUT or ref.M < 1000
    out = Out(b, N, 3)
    dn, dr, ds = _dev(n), _dev(r), _dev(sh)
    keep = [x.clone() for x in (dn, dr, ds)]
    _lib.check(_lib.lib().texir_generate_dir(_lib.ptr(dn), _lib.ptr(dr) if mode == "importance" else None, _lib.ptr(ds), b, N, MODE_ID[mode], _lib.ptr(out.t),
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    for x, k in zip((dn, dr, ds), keep):
        assert torch.equal(x.view(torch.int32), k.view(torch.int32))
    got = out.get().reshape(-1, 3)
    for k in range(3):
        SC.check_value(got[:, k], ref, "d%d" % k, "gen-" + mode, "b %d N %d component %d" % (b, N, k))


@pytest.mark.parametrize("mode", ["uniform", "cosine", "importance"])
def test_generate_dir(mode):
    for b in (1, 3, 11):
        for N in (1, 2, 3, 16, 64, 100, 1000, 2048):
            run_gen_dir(mode, b, N)
    for N in ((1, 2, 3, 16, 64, 100, 1000) if mode == "importance" else (3, 64, 1000)):
        run_gen_dir(mode, 257, N)


def test_generate_dir_grid_stride_round():
    """b * N above 2048 blocks of 256: the grid-stride round runs"""
    assert 257 * 2048 > 2048 * 256
    run_gen_dir("importance", 257, 2048)


def test_zz_record():
    """prints the record the module docstring keeps (run last)"""
    for k in sorted(SC.RATIOS):
        print("RECORD ratio %-22s %.3f" % (k, SC.RATIOS[k]))
    for k in sorted(SC.SHARES):
        print("RECORD share %-22s multi %.4f left %.5f nonbase %.5f" % (k, SC.SHARES[k]["multi"], SC.SHARES[k]["left"], SC.SHARES[k]["nonbase"]))
