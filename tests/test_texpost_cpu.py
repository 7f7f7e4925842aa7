"""CPU: the pad + denoise step between the stages (texir_code_amd/texpost.py, csrc/texpost.hip) -- what can be checked without a GPU: the C-ABI
surface, the index tables of the `reference` mode against F.grid_sample itself, the runner's conf keys, and the guided torch path of
tools.denoise_atrous (bit-identity of its default call with the function as it was, and two exact identities of the guides)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from texpost_cases import noisy_lowpass, seeded_image

@pytest.fixture(autouse=True)
def _one_torch_thread():
    """the torch filter is thousands of tiny elementwise ops on small images: one host thread (elementwise: the values do not depend on it)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


ENTRY_POINTS = ("texir_texture_pad_workspace_bytes", "texir_texture_pad", "texir_texture_denoise")


def test_header_declares_and_library_exports_the_entry_points():
    from texir_code_amd import _lib
    txt = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    declared = set(re.findall(r"TEXIR_API\s+[\w\s\*]+?\b(texir_\w+)\s*\(", txt))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for s in ENTRY_POINTS:
        assert s in declared, "include/texir_hip.h does not declare %s" % s
        assert hasattr(L, s), "libtexir_hip.so does not export %s" % s
    assert "padding_texture.py:49-87" in txt
    assert L.texir_texture_pad_workspace_bytes(96, 128) >= 96 * 128 * 4


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 100, 124, 1000, 1024, 2048, 4095, 4096, 8192])
def test_reference_index_map_is_what_grid_sample_reads(n):
    from texir_code_amd import texpost
    m = texpost.reference_index_map(n)
    assert m.dtype == np.int32 and m.shape == (n,)
    # a 1 x n image holding index + 1, sampled at the coordinates tools.padding_texture forms for source index i (zero padding -> 0 -> -1)
    img = (torch.arange(n, dtype=torch.float32) + 1).reshape(1, 1, 1, n)
    u = torch.arange(n).float() / torch.tensor([n]) * 2.0 - 1.0
    grid = torch.stack([u, torch.zeros(n)], -1).reshape(1, 1, n, 2)
    got = F.grid_sample(img, grid, mode="nearest", align_corners=False)[0, 0, 0].numpy().astype(np.int64) - 1
    assert np.array_equal(m, got)
    # and along y (the same arithmetic on the other axis)
    grid_y = torch.stack([torch.zeros(n), u], -1).reshape(1, n, 1, 2)
    got_y = F.grid_sample(img.reshape(1, 1, n, 1), grid_y, mode="nearest", align_corners=False)[0, 0, :, 0].numpy().astype(np.int64) - 1
    assert np.array_equal(m, got_y)


def test_reference_mode_leaves_a_third_of_the_holes_black():
    """finding 2 of the step's design, pinned on the CPU tool the `reference` mode reproduces: grid_sample's rounding reads odd sources one texel low"""
    pytest.importorskip("scipy")
    from texir_code_amd import tools
    for (h, w), lo in (((96, 128), 0.30), ((100, 124), 0.33)):
        img, valid = seeded_image(h, w)
        out = tools.padding_texture(img)
        black = (out[~valid].sum(-1) == 0).mean()
        assert lo < black < lo + 0.06, black


def test_runner_rejects_bad_values_of_the_two_keys():
    from texir_code_amd import conf as C
    from texir_code_amd.trainer.generate_ir_texture import irt_post_settings
    cf = lambda body: C.parse_string("train{\n%s\n}" % body)
    assert irt_post_settings(cf("batch_size = 1")) == ("none", "none", (0.5, 0.3, 0.25))
    assert irt_post_settings(cf("irt_pad = nearest\nirt_denoise = guided\nirt_denoise_sigma = [0.4, 0.2, 0]")) == ("nearest", "guided", (0.4, 0.2, 0.0))
    assert irt_post_settings(cf("irt_pad = reference"))[:2] == ("reference", "none")
    for bad in ("irt_pad = closest", "irt_pad = nearest\nirt_denoise = oidn", "irt_denoise = color", "irt_pad = none\nirt_denoise = guided",
                "irt_pad = nearest\nirt_denoise_sigma = [0.5, 0.3]", "irt_pad = nearest\nirt_denoise_sigma = [0, 0.3, 0.25]"):
        with pytest.raises(ValueError):
            irt_post_settings(cf(bad))


def _denoise_atrous_before(img, iterations=3, sigma_c=0.5, device=None):
    """tools.denoise_atrous as it stood before the guides were added (kept verbatim: the default call must not move by a bit)"""
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    x = torch.as_tensor(np.asarray(img, np.float32), device=device)
    valid = (x.sum(-1, keepdim=True) != 0).float()
    c = torch.log1p(x.clamp(min=0))
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=device) / 16.0
    H, W, _ = c.shape
    for it in range(iterations):
        step, s2 = 1 << it, (sigma_c * 0.5 ** it) ** 2
        acc, wsum = torch.zeros_like(c), torch.zeros((H, W, 1), device=device)
        pad = 2 * step
        cp = F.pad(c.permute(2, 0, 1)[None], (pad, pad, pad, pad), mode="replicate")[0].permute(1, 2, 0)
        vp = F.pad(valid.permute(2, 0, 1)[None], (pad, pad, pad, pad), mode="constant", value=0.0)[0].permute(1, 2, 0)
        for dy in range(5):
            for dx in range(5):
                q = cp[dy * step:dy * step + H, dx * step:dx * step + W]
                w = k1[dy] * k1[dx] * torch.exp(-((q - c) ** 2).sum(-1, keepdim=True) / s2) * vp[dy * step:dy * step + H, dx * step:dx * step + W]
                acc += q * w
                wsum += w
        c = torch.where(valid > 0, acc / wsum.clamp(min=1e-20), c)
    return (torch.expm1(c) * valid).cpu().numpy()


def test_denoise_atrous_default_call_is_bit_identical_to_before():
    from texir_code_amd import tools
    img = noisy_lowpass(64, 96)
    for it in (1, 3, 4):
        a = _denoise_atrous_before(img, iterations=it, device="cpu")
        b = tools.denoise_atrous(img, iterations=it, device="cpu")
        assert a.tobytes() == b.tobytes(), it
    a = _denoise_atrous_before(img, sigma_c=0.3, device="cpu")
    assert a.tobytes() == tools.denoise_atrous(img, sigma_c=0.3, device="cpu").tobytes()


def test_guided_torch_path_identities_hold_exactly():
    from texir_code_amd import tools
    h, w = 64, 96
    img = noisy_lowpass(h, w)
    plain = tools.denoise_atrous(img, device="cpu")
    # constant guides add exactly 0 to every exponent
    const = np.broadcast_to(np.array([0.3, -0.2, 0.9], np.float32), (h, w, 3)).copy()
    assert np.array_equal(tools.denoise_atrous(img, device="cpu", guide_nrm=const, guide_pos=const), plain)
    # two half-planes with orthogonal normals and sigma_n = 0.1: every cross-half weight is exp(-(E + 200)) = 0 in float32, so the left half is
    # filtered as if the right half were holes
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:, :w // 2, 0] = 1.0
    nrm[:, w // 2:, 1] = 1.0
    cut = img.copy()
    cut[:, w // 2:] = 0.0
    got = tools.denoise_atrous(img, device="cpu", guide_nrm=nrm, sigma_n=0.1)
    want = tools.denoise_atrous(cut, device="cpu")
    assert np.array_equal(got[:, :w // 2], want[:, :w // 2])
    # and the guide does something: the right half is no longer the colour-only result everywhere near the cut
    assert not np.array_equal(got, plain)
