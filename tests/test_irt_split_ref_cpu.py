"""CPU: the reference of the irradiance split (irt_split_cases) is sharp enough to bind, accepts a float32 restatement of the documented rule and rejects the
ways a split can go wrong; the numpy helpers of texir_code_amd/irtsplit.py; the C-ABI declares and binds the two entry points.

  * the caps of trace_cases (no overflowing ray, samples with more than one outcome <= 2 %, texels that are not sharp <= 20 %) hold for every reference the
    GPU module uses: the masked textures of `lamp` and `bands` at 130 texels x 64 samples and 70 x 512;
  * split_f32 -- trace_f32's hits, shade_f32 on the texture hdr * [label == k], estimator_f32 in the 64-texel form -- lies inside every class's intervals;
  * one label for the whole footprint, labels upside down, labels transposed, a class index off by one and labels >= K folded into the last class fall out.
"""
import os
import re

import numpy as np
import pytest

import irt_split_cases as SP
import trace_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,n_tex,N", SP.REF_CASES, ids=["%s_%dx%d" % c for c in SP.REF_CASES])
def test_caps_of_the_gpu_split_references(name, n_tex, N):
    K, _ = SP.labels(name)
    for k in range(K):
        over, multi, unsharp = SP.split_ref(name, k, n_tex, N).caps()
        print("caps %s class %d %dx%d: overflow %d, samples with more than one outcome %.4f, texels not sharp %.3f" % (name, k, n_tex, N, over, multi, unsharp))
        assert over == 0 and multi <= TC.CAP_MULTI and unsharp <= TC.CAP_UNSHARP
        SP._REF.pop((name, k, n_tex, N))                        # (the references are large)


_TR = {}


def traced():
    if not _TR:
        _TR["v"] = SP.traced(*SP.CPU_CASE)
    return _TR["v"]


@pytest.mark.parametrize("name", ["lamp", "bands"])
def test_float32_restatement_is_accepted_per_class(name):
    c, d, t, pid, uv = traced()
    K, lab = SP.labels(name)
    got = SP.split_f32(c, d, t, pid, uv, lab, K)
    parts = TC.n_parts(c.N, "group")
    for k in range(K):
        ref = SP.split_ref(name, k, *SP.CPU_CASE)
        over, multi, unsharp = ref.caps()
        assert over == 0 and multi <= TC.CAP_MULTI and unsharp <= TC.CAP_UNSHARP
        ref.check(got[k], "group", parts, "split_f32", "%s class %d" % (name, k))
    # the classes are a partition of the texture: their sum is the plain estimator's value up to the roundings of K sums
    full = TC.estimator_f32(c.nrm[c.ids], d, TC.shade_f32(c.geo, t, pid, uv).reshape(len(c.ids), c.N, 3), False, "group", parts)
    assert np.allclose(got.astype(np.float64).sum(0), full, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("mut", SP.MUTANTS)
def test_split_mutants_are_rejected(mut):
    c, d, t, pid, uv = traced()
    name = SP.MUTANT_LABELS[mut]
    K, lab = SP.labels(name)
    good, bad = SP.split_f32(c, d, t, pid, uv, lab, K), SP.split_f32(c, d, t, pid, uv, lab, K, mut)
    parts = TC.n_parts(c.N, "group")
    hit = []
    for k in range(K):
        ref = SP.split_ref(name, k, *SP.CPU_CASE)
        ref.check(good[k], "group", parts, "split_f32", "%s class %d (before %s)" % (name, k, mut))
        hit.append(TC.rejected(ref.check, bad[k], "group", parts, "mutant", "%s %s class %d" % (mut, name, k)))
    assert any(hit), (mut, name, hit)


def test_labels_from_radiance_is_the_reference_rule():
    from texir_code_amd import irtsplit
    geo, _ = TC.golden_geo(SP.SCENE)
    for exposure in (0.0, 2.0, -1.5):
        tex = geo.hdr * np.float32(2.0 ** exposure)
        t = tex * np.float32(2.0 ** -exposure)
        want = ((np.float32(0.299) * t[..., 0] + np.float32(0.587) * t[..., 1] + np.float32(0.114) * t[..., 2]) > np.float32(0.5)).astype(np.uint8)
        got = irtsplit.labels_from_radiance(tex, exposure)
        assert got.dtype == np.uint8 and got.shape == tex.shape[:2] and np.array_equal(got, want)
    K, lamp = SP.labels("lamp")
    assert K == 2 and 0.02 < lamp.mean() < 0.04                 # the room's lamp: 2.8 % of the texels
    assert np.array_equal(irtsplit.labels_from_radiance(geo.hdr, 0.0, threshold=1e30), np.zeros_like(lamp))


def test_labels_from_seg():
    from texir_code_amd import irtsplit
    seg = np.array([[45, 46, 7], [0, 45, 255]], np.uint8)
    assert np.array_equal(irtsplit.labels_from_seg(seg, {45: 1, 46: 2}), np.array([[1, 2, 0], [0, 1, 0]], np.uint8))
    assert irtsplit.labels_from_seg(seg, {}).sum() == 0
    with pytest.raises(ValueError):
        irtsplit.labels_from_seg(seg, {45: 256})


def test_combine_and_replace_constant_on_hand_made_arrays():
    import torch
    from texir_code_amd import irtsplit
    E = np.array([[[1.0, 2.0, 3.0], [0.0, 1.0, 0.0]], [[10.0, 20.0, 30.0], [4.0, 0.0, 0.5]]], np.float32)            # [K=2, texels=2, 3]
    F = np.array([[[0.5, 0.5, 0.5], [1.0, 1.0, 1.0]], [[0.25, 0.25, 0.25], [2.0, 2.0, 2.0]]], np.float32)
    assert np.array_equal(irtsplit.combine(E, [1.0, 1.0]), E[0] + E[1])
    assert np.array_equal(irtsplit.combine(E, [2.0, 0.0]), 2 * E[0])
    assert np.array_equal(irtsplit.combine(E, [(1.0, 0.0, 2.0), 0.5]), np.array([[6.0, 10.0, 21.0], [2.0, 0.0, 0.25]], np.float32))
    assert np.array_equal(irtsplit.replace_constant(E, F, 1, (2.0, 4.0, 8.0)), np.array([[1.5, 3.0, 5.0], [4.0, 9.0, 16.0]], np.float32))
    assert np.array_equal(irtsplit.replace_constant(E, F, 0, 0.0), E[1])
    got = irtsplit.combine(torch.from_numpy(E), [(1.0, 0.0, 2.0), 0.5])
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), irtsplit.combine(E, [(1.0, 0.0, 2.0), 0.5]))
    assert np.array_equal(irtsplit.replace_constant(torch.from_numpy(E), torch.from_numpy(F), 1, (2.0, 4.0, 8.0)).numpy(), irtsplit.replace_constant(E, F, 1, (2.0, 4.0, 8.0)))
    with pytest.raises(ValueError):
        irtsplit.combine(E, [1.0])
    with pytest.raises(ValueError):
        irtsplit.replace_constant(E, F, 2, 1.0)


def test_header_declares_and_lib_binds_the_entry_points():
    import ctypes as C
    from texir_code_amd import _lib
    txt = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    assert re.search(r"TEXIR_API\s+int64_t\s+texir_irt_split_workspace_bytes\s*\(\s*int64_t\s+n_ids,\s*int32_t\s+N,\s*int32_t\s+K\s*\)", txt)
    assert re.search(r"TEXIR_API\s+int\s+texir_irt_split\s*\(", txt)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.texir_irt_split_workspace_bytes.restype is C.c_int64 and len(L.texir_irt_split.argtypes) == 16
    # 12 bytes x K x parts per listed texel; the plan of the 64-texel form: N = 2048 -> 32 parts, 64 -> 8, 100 -> 1
    assert L.texir_irt_split_workspace_bytes(64, 2048, 8) == 12 * 64 * 8 * 32
    assert L.texir_irt_split_workspace_bytes(130, 64, 3) == 12 * 130 * 3 * TC.n_parts(64, "group")
    assert L.texir_irt_split_workspace_bytes(7, 100, 1) == 12 * 7
    assert L.texir_irt_split_workspace_bytes(7, 100, 9) == 0 and L.texir_irt_split_workspace_bytes(7, 0, 2) == 0


def test_workspace_bytes_follow_the_switches_of_the_plan(monkeypatch):
    """the split's parts per texel are irt_plan's: the same function of N, TEXIR_IRT_MIN_PART_CELLS and TEXIR_IRT_LOG2PARTS (trace_cases.n_parts restates it)"""
    from texir_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    monkeypatch.setenv("TEXIR_IRT_MIN_PART_CELLS", "64")        # (the fixture calls texir_reload_env after every change, and once more after undoing them)
    assert TC.n_parts(512, "group", min_part_cells=64) == 8
    assert L.texir_irt_split_workspace_bytes(130, 512, 3) == 12 * 130 * 3 * TC.n_parts(512, "group", min_part_cells=64)
    monkeypatch.delenv("TEXIR_IRT_MIN_PART_CELLS")
    monkeypatch.setenv("TEXIR_IRT_LOG2PARTS", "0")
    assert L.texir_irt_split_workspace_bytes(130, 512, 3) == 12 * 130 * 3


def test_relight_irt_command_on_hand_made_files(tmp_path):
    """values an RGBE file holds exactly (8-bit mantissas under one power of two): the command's arithmetic shows through the files unrounded"""
    from texir_code_amd import io_formats as IO, tools
    d = str(tmp_path)
    E0 = np.zeros((4, 6, 3), np.float32)
    E0[..., 0], E0[..., 1], E0[1, 2] = 0.5, 0.25, (1.0, 0.5, 0.75)
    E1 = np.full((4, 6, 3), 0.125, np.float32)
    F1 = np.full((4, 6, 3), 0.25, np.float32)
    assert tools.main(["relight-irt", d, "--class", "0", "--colour", "1,1,1"]) == 1                          # no class files
    for name, a in (("class0", E0), ("class1", E1), ("unit1", F1)):
        IO.write_hdr(os.path.join(d, "0_irr_texture_%s.hdr" % name), a)
    assert tools.main(["relight-irt", d, "--class", "2", "--colour", "1,1,1"]) == 2                          # no such class
    assert tools.main(["relight-irt", d, "--class", "1"]) == 2 and tools.main(["relight-irt", d, "--class", "1", "--colour", "1,2"]) == 2
    dst = os.path.join(d, "0_irr_texture_relit.hdr")
    assert not os.path.exists(dst)
    assert tools.main(["relight-irt", d, "--class", "1", "--colour", "2,0,4"]) == 0
    assert np.array_equal(IO.read_hdr(dst), E0 + E1 * np.array([2.0, 0.0, 4.0], np.float32))
    before = open(dst, "rb").read()
    assert tools.main(["relight-irt", d, "--class", "1", "--colour", "1,1,1"]) == 1 and open(dst, "rb").read() == before      # refuses to overwrite
    os.remove(dst)
    assert tools.main(["relight-irt", d, "--class", "1", "--colour", "2,1,0.5", "--replace"]) == 0
    assert np.array_equal(IO.read_hdr(dst), E0 + F1 * np.array([2.0, 1.0, 0.5], np.float32))
    os.remove(dst)
    assert tools.main(["relight-irt", d, "--class", "0", "--colour", "1,1,1", "--replace"]) == 1              # no unit file of class 0
