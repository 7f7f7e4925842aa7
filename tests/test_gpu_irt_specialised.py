"""The fixed instantiations of the 64-texel IrT kernel (csrc/kernels.hip IrtFixed: N a power of two, sampling mode and estimator, texture layout 4 and the
float node copy known at compile time) against the generic kernel, bit for bit, and the launcher's choice between them.

Scene: a ~2 000-triangle room whose radiance texture is RGBE-born (layout 4); 209 listed texels of a 32 x 32 texel G-buffer -- three full 64-texel groups
and a partial one, so the last wave has dead lanes -- one of them with a zero normal and one with |n.x| > 0.99 (make_frame's special arms).  The 64-texel
form is forced (TEXIR_IRT_TEXELS_PER_WAVE=64).  TEXIR_IRT_SPECIALISE is read when the library loads, so each setting runs in a child process of its own
(tests/irt_specialised_worker.py, both started together, once per session); a case below compares what the two wrote.

The kernel FORM (irt_kernel_name) is the same under both settings; irt_kernel_variant names the instantiation: the fixed one where the call is what it
was compiled for, the form's generic kernel otherwise -- N = 48, a float-valued texture (layout 2), a scene without float nodes, and every call under
TEXIR_IRT_SPECIALISE=0."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GROUP = "irt_group_kernel<false, 4, 6>"
FIXED = "irt_group_kernel<false, 4, 6, IrtFixed<%d, %s>>"
_RUNS = {}


def runs(tmp_path_factory):
    """{setting: the worker's arrays} for TEXIR_IRT_SPECIALISE = "1" and "0" """
    if not _RUNS:
        d = tmp_path_factory.mktemp("irt_specialised")
        procs = {}
        # (the cases rely on the launcher's default plan -- 8 parts at N = 64, one at N = 8: no plan switch of the caller's environment reaches the children)
        base = {k: v for k, v in os.environ.items() if k not in ("TEXIR_IRT_MIN_PART_CELLS", "TEXIR_IRT_LOG2PARTS", "TEXIR_IRT_REFILL", "TEXIR_TEX_LAYOUT",
                                                                   "TEXIR_UNIFORM_FLOAT", "TEXIR_BVH_WIDTH")}
        try:
            for s in ("1", "0"):
                env = dict(base, TEXIR_IRT_SPECIALISE=s, TEXIR_IRT_TEXELS_PER_WAVE="64")
                procs[s] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "irt_specialised_worker.py"), str(d / ("spec%s.npz" % s))],
                                            cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for s, p in procs.items():
                log = p.communicate(timeout=300)[0]
                assert p.returncode == 0, "worker with TEXIR_IRT_SPECIALISE=%s: exit %s\n%s" % (s, p.returncode, log[-3000:])
        finally:
            for p in procs.values():                 # whatever happened above, no child keeps the GPU open behind a failed test
                if p.poll() is None:
                    p.kill()
                p.wait()
        for s in procs:
            with np.load(d / ("spec%s.npz" % s)) as z:
                _RUNS[s] = {k: z[k] for k in z.files}
    return _RUNS


def both(tmp_path_factory, case):
    r = runs(tmp_path_factory)
    a, b = torch.from_numpy(r["1"]["irr/" + case]), torch.from_numpy(r["0"]["irr/" + case])
    assert a.shape == (209, 3) and bool(torch.isfinite(a).all())
    assert float(a.abs().max()) > 0.0                        # (the room is lit: the comparison is not one of zeros)
    names = {s: (str(r[s]["form/" + case]), str(r[s]["variant/" + case])) for s in ("1", "0")}
    return a, b, names


@pytest.mark.parametrize("N", [64, 8])
@pytest.mark.parametrize("mode,estimator", [("uniform", False), ("cosine", False), ("cosine", True)])
def test_fixed_kernel_equals_the_generic_one(tmp_path_factory, N, mode, estimator):
    """N = 64: 8 parts and the combine kernel; N = 8: one part, the kernel writes the irradiance itself"""
    case = "packed_%s_%d" % ("estimator" if estimator else mode, N)
    a, b, names = both(tmp_path_factory, case)
    assert names["1"] == (GROUP, FIXED % (0 if mode == "uniform" else 1, "true" if estimator else "false"))
    assert names["0"] == (GROUP, GROUP)
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["packed_uniform_48", "floats_uniform_64", "quantised_uniform_64"])
def test_calls_the_fixed_kernel_was_not_compiled_for_take_the_generic_one(tmp_path_factory, case):
    """N not a power of two; texture layout 2; a scene built with TEXIR_UNIFORM_FLOAT=0"""
    a, b, names = both(tmp_path_factory, case)
    assert names["1"] == (GROUP, GROUP) and names["0"] == (GROUP, GROUP)
    assert torch.equal(a, b)


def test_the_frames_special_arms_are_among_the_compared_texels(tmp_path_factory):
    """the zero-normal texel gathers nothing (its rays have no direction); the texel with |n.x| > 0.99 gathers light through the other axis choice"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import irt_specialised_worker as W
    for case in ("packed_uniform_64", "packed_cosine_8"):
        a, b, _ = both(tmp_path_factory, case)
        assert bool((a[W.ZERO_NORMAL] == 0).all()) and bool((a[W.AXIS_NORMAL] > 0).any())
        assert torch.equal(a[[W.ZERO_NORMAL, W.AXIS_NORMAL]], b[[W.ZERO_NORMAL, W.AXIS_NORMAL]])


def test_counting_launch_reports_the_generic_kernels_counters(tmp_path_factory):
    """stats=True: rays, node fetches, triangle tests and hits of the call, and its irradiance"""
    a, b, _ = both(tmp_path_factory, "counted_uniform_64")
    r = runs(tmp_path_factory)
    sa, sb = r["1"]["stats/counted_uniform_64"], r["0"]["stats/counted_uniform_64"]
    assert sa[0] == 209 * 64 and sa[1] > 0 and sa[2] > 0 and 0 < sa[3] <= sa[0]
    assert np.array_equal(sa, sb)
    assert torch.equal(a, b)
    # ... and the counted launch computes what the plain one does, under either setting
    for s in ("1", "0"):
        assert np.array_equal(r[s]["irr/counted_uniform_64"], r[s]["irr/packed_uniform_64"])
