"""Seeded inputs and brute-force helpers shared by test_texpost_cpu.py and test_gpu_texpost.py (no tests here).  Everything is drawn from torch's
CPU generators, so both machines see identical arrays."""
import numpy as np
import torch
import torch.nn.functional as F


def seeded_mask(h, w, cell=8, seed=666, thresh=0.42):
    """validity mask of an atlas-like image: a thresholded bicubic upsampling of uniform noise on a (h/cell + 2) x (w/cell + 2) grid"""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(1, 1, h // cell + 2, w // cell + 2, generator=g)
    return F.interpolate(z, size=(h, w), mode="bicubic", align_corners=False)[0, 0] > thresh, z


def seeded_image(h, w, cell=8):
    """[h,w,3] float32 numpy: values in [0.25, 1.25) on valid texels, exactly 0 on holes; + the bool validity mask"""
    valid, _ = seeded_mask(h, w, cell)
    v = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)) + 0.25
    return (v * valid[..., None]).numpy().astype(np.float32), valid.numpy()


def hole_mask(img):
    """the reference's rule (tools/padding_texture.py:54-56): float32 channel sum in channel order == 0"""
    s = img[..., 0].astype(np.float32)
    for c in range(1, img.shape[-1]):
        s = (s + img[..., c]).astype(np.float32)
    return s == 0.0


def brute_force(img):
    """all hole x all valid squared distances in int64 -> (hy, hx, vy, vx, d2 [n_hole, n_valid], dmin [n_hole])"""
    hole = hole_mask(img)
    hy, hx = np.nonzero(hole)
    vy, vx = np.nonzero(~hole)
    d2 = (hy[:, None].astype(np.int64) - vy[None]) ** 2 + (hx[:, None].astype(np.int64) - vx[None]) ** 2
    return hy, hx, vy, vx, d2, d2.min(1)


def noisy_lowpass(h, w, hole_frac=0.1, seed=3):
    """a noisy low-pass HDR-like image with a share of zero texels (the denoiser's input)"""
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.rand(1, 3, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)
    img = (low.clamp(min=0.02) * 2.0) * (1.0 + 0.3 * torch.randn(h, w, 3, generator=g)).clamp(min=0.05)
    img = img * (torch.rand(h, w, 1, generator=g) >= hole_frac)
    return img.numpy().astype(np.float32)


def seeded_guides(h, w, seed=5):
    """smooth unit normals and positions (texel coordinates + a smooth height)"""
    g = torch.Generator().manual_seed(seed)
    zz = F.interpolate(torch.rand(1, 1, h // 16 + 2, w // 16 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)[0, 0]
    gy, gx = torch.gradient(zz * 8.0)
    n = torch.stack([-gx, -gy, torch.ones_like(zz)], -1)
    n = n / n.norm(dim=-1, keepdim=True)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    p = torch.stack([xx / w, yy / h, zz * 0.1], -1)
    return n.numpy().astype(np.float32), p.numpy().astype(np.float32)
