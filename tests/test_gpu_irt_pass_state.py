"""The per-texel state a pass of the fixed 64-texel IrT kernels reloads from its parked record (csrc/kernels.hip Parked: frame, shifts, raw normal, cell
offsets; 1 / N built from log2 N) against the generic kernel, which keeps the chunk's own values: bit for bit, for the three fixed instantiations.

Scene and list are tests/test_gpu_irt_specialised.py's: the ~2 000-triangle room with an RGBE-born texture (layout 4), 209 listed texels -- three full groups
and a partial one, one texel with a zero normal and one with |n.x| > 0.99 -- and TEXIR_IRT_TEXELS_PER_WAVE=64.  One child process per setting of
TEXIR_IRT_SPECIALISE (tests/irt_pass_state_worker.py, both started together, once per session); a case below compares what the two wrote.

Cases: N = 1, 2, 16, 512, 2048 (one part to 32 parts; both ends of the exponent of 1 / N and the bench's own N); lists of 5 and of exactly 64 texels; texels
whose shifts are 0.0 and 1 - 2^-24 (the cell offsets wrap); the persistent grid capped at ONE block, so that every wave runs many chunks in turn and a
record left over from the previous chunk would show; the same call twice.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GROUP = "irt_group_kernel<false, 4, 6>"
FIXED = {"uniform": "irt_group_kernel<false, 4, 6, IrtFixed<0, false>>", "cosine": "irt_group_kernel<false, 4, 6, IrtFixed<1, false>>",
         "estimator": "irt_group_kernel<false, 4, 6, IrtFixed<1, true>>"}
INSTANTIATIONS = ("uniform", "cosine", "estimator")
_RUNS = {}


def runs(tmp_path_factory):
    """{setting: the worker's arrays} for TEXIR_IRT_SPECIALISE = "1" and "0" """
    if not _RUNS:
        d = tmp_path_factory.mktemp("irt_pass_state")
        procs = {}
        base = {k: v for k, v in os.environ.items() if k not in ("TEXIR_IRT_MIN_PART_CELLS", "TEXIR_IRT_LOG2PARTS", "TEXIR_IRT_REFILL", "TEXIR_TEX_LAYOUT",
                                                                   "TEXIR_UNIFORM_FLOAT", "TEXIR_BVH_WIDTH", "TEXIR_IRT_GRID_CAP")}
        try:
            for s in ("1", "0"):
                env = dict(base, TEXIR_IRT_SPECIALISE=s, TEXIR_IRT_TEXELS_PER_WAVE="64")
                procs[s] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "irt_pass_state_worker.py"), str(d / ("state%s.npz" % s))],
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
            with np.load(d / ("state%s.npz" % s)) as z:
                _RUNS[s] = {k: z[k] for k in z.files}
    return _RUNS


def both(tmp_path_factory, case, inst, listed=209):
    """the fixed kernel's and the generic kernel's irradiance of a case, after the checks every case shares"""
    r = runs(tmp_path_factory)
    a, b = torch.from_numpy(r["1"]["irr/" + case]), torch.from_numpy(r["0"]["irr/" + case])
    assert a.shape == (listed, 3) and b.shape == (listed, 3) and bool(torch.isfinite(a).all())
    assert str(r["1"]["variant/" + case]) == FIXED[inst] and str(r["0"]["variant/" + case]) == GROUP
    return a, b


@pytest.mark.parametrize("N", [1, 2, 16, 512, 2048])
@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_every_sample_count_gives_the_generic_kernels_bits(tmp_path_factory, inst, N):
    a, b = both(tmp_path_factory, "all_%s_%d" % (inst, N), inst)
    if N >= 16:
        assert float(a.abs().max()) > 0.0                    # (the room is lit: the comparison is not one of zeros)
    assert torch.equal(a, b)


@pytest.mark.parametrize("listed", [5, 64])
@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_short_lists_give_the_generic_kernels_bits(tmp_path_factory, inst, listed):
    """a partial group alone (59 dead lanes); exactly one full group"""
    a, b = both(tmp_path_factory, "list%d_%s_64" % (listed, inst), inst, listed)
    assert float(a.abs().max()) > 0.0
    assert torch.equal(a, b)
    # ... and a texel's irradiance does not depend on what else is listed
    full, _ = both(tmp_path_factory, "all_%s_64" % inst, inst)
    assert torch.equal(a, full[:listed])


@pytest.mark.parametrize("N", [64, 2048])
@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_shifts_at_the_edges_of_the_unit_interval_wrap_alike(tmp_path_factory, inst, N):
    """the first eight listed texels carry shifts of 0.0, 0.5 and 1 - 2^-24 in both components"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import irt_pass_state_worker as W
    a, b = both(tmp_path_factory, "edge_%s_%d" % (inst, N), inst)
    assert float(a[:W.N_EDGE].abs().max()) > 0.0
    assert torch.equal(a, b)
    if N == 64:      # the edge shifts matter: those texels differ from the run with the generator's shifts, the others do not
        plain, _ = both(tmp_path_factory, "all_%s_64" % inst, inst)
        assert not torch.equal(a[:W.N_EDGE], plain[:W.N_EDGE]) and torch.equal(a[W.N_EDGE:], plain[W.N_EDGE:])


@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_one_block_running_every_chunk_in_turn(tmp_path_factory, inst):
    """TEXIR_IRT_GRID_CAP=1: four waves share the 32 chunks; the result is that of the full grid"""
    a, b = both(tmp_path_factory, "oneblock_%s_64" % inst, inst)
    assert torch.equal(a, b)
    full, _ = both(tmp_path_factory, "all_%s_64" % inst, inst)
    assert torch.equal(a, full)


@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_the_same_call_twice_gives_equal_bits(tmp_path_factory, inst):
    first, b = both(tmp_path_factory, "again_%s_64" % inst, inst)
    second, _ = both(tmp_path_factory, "all_%s_64" % inst, inst)
    assert torch.equal(first, second) and torch.equal(first, b)


def test_the_frames_special_arms_are_among_the_compared_texels(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import irt_specialised_worker as S
    for inst in INSTANTIATIONS:
        a, b = both(tmp_path_factory, "all_%s_2048" % inst, inst)
        assert bool((a[S.ZERO_NORMAL] == 0).all()) and bool((a[S.AXIS_NORMAL] > 0).any())
        assert torch.equal(a[[S.ZERO_NORMAL, S.AXIS_NORMAL]], b[[S.ZERO_NORMAL, S.AXIS_NORMAL]])
