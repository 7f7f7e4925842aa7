"""GPU: the WHOLE textured material-estimation step of the product -- ray-cast G-buffer -> trilinear-mip texture fetch (HIP) -> fused GGX
specular trace -> fused loss -> gather backward over per-view tap lists -> deferred mip folds -> sparse level-0 gradient -> fused Adam with
clamps, eagerly and through hipGraph replay -- against oracle/mat_step.py: an independent plain-torch-autograd restatement of
models/mat_nvdiffrast.py:107-190,201-279 + models/loss.py:81-115,214-295 + trainer/train_material.py:416-593 on a RASTERISED G-buffer
(oracle/raster.py), lit by the C oracle's own tracer, stepped by torch.optim.Adam.  The oracle's render and loss restatements are pinned
to the reference's own outputs and autograd gradients on the CPU (tests/test_mat_step_oracle.py).

Tolerances: north_star's 1e-3 relative L2 on gradients asserted, with the tighter observed bound next to it."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

LR = 3e-2
_OGB = {}          # the oracle's rasterised G-buffers (c, view) -> dict: independent of the texture sizes, ~15 s of numpy each


@pytest.fixture(autouse=True)
def _bounded_host_threads():
    """the oracle side is hundreds of small torch-CPU ops and small OpenMP regions of the C oracle: on a 256-thread host two full-width thread pools
    (torch's OpenMP runtime and the oracle library's) spin against each other and the test takes minutes instead of seconds"""
    from oracle import oracle as O
    before = torch.get_num_threads()
    n = max(1, min(16, os.cpu_count() or 1))
    torch.set_num_threads(n)
    O.set_num_threads(n)
    yield
    torch.set_num_threads(before)


def _smooth_radiance(res, seed=5):
    """a radiance texture without step edges: a low-pass random field, 0.5 x (1 +- 0.05) per channel, the same statistics over the whole atlas.
    The radiance a specular ray returns is then continuous in its direction up to the 10 % a chart border can jump -- not the three orders of magnitude of a lamp edge
    -- so a ray falling on the other side of an edge in the product than in the oracle moves a gradient by ~1e-5 of its norm, and NO texel needs setting aside."""
    rng = np.random.default_rng(seed)
    n = res // 16 + 2
    coarse = torch.from_numpy(rng.uniform(-1.0, 1.0, (1, 3, n, n)).astype(np.float32))
    field = torch.nn.functional.interpolate(coarse, size=(res, res), mode="bicubic", align_corners=True)[0].permute(1, 2, 0)
    return (0.5 * (1.0 + 0.05 * field.clamp(-1.0, 1.0))).contiguous().numpy()


def _world(golden, c, ra, rr, seed=11, smooth=False, view_keys=("v0", "v1")):
    from oracle import mat_step as MS, oracle as O
    from texir_code_amd import cameras, conf as C, gbuffer as GB
    from texir_code_amd.models import MaterialModel
    from texir_code_amd.scene import Scene
    from texir_code_amd.trainer.train_material import build_masks
    g = golden("irt_room.npz")
    verts, tris, tri_uvs, hdr = g["verts"], g["tris"], g["tri_uvs"], g["hdr"]
    if smooth:
        hdr = _smooth_radiance(hdr.shape[0])
    rng = np.random.default_rng(seed)
    fn = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]])
    fn /= np.maximum(np.linalg.norm(fn, axis=-1, keepdims=True), 1e-20)
    cn = (np.repeat(fn, 3, axis=0) + 0.08 * rng.normal(size=(3 * tris.shape[0], 3))).astype(np.float32)      # smooth-ish, NOT unit (raw-normal dots)
    sc = Scene(verts, tris, tri_uvs, hdr, device=0)
    GB.set_corner_normals(sc, cn)
    osc = O.Scene(verts, tris, tri_uvs, hdr)
    cf = C.parse_string("train{ pano_img_res = [%d,%d]\n sample_light = [64,16]\n hdr_exposure = 0 }\nmodels{ render{ sample_type = [uniform, importance] } }" % (2 * c, 4 * c))
    gen = torch.Generator().manual_seed(seed)
    irrt = torch.rand(128, 128, 3, generator=gen) + 0.3
    a0 = 0.2 + 0.6 * torch.rand(ra, ra, 3, generator=gen)
    r0 = 0.1 + 0.5 * torch.rand(rr, rr, 1, generator=gen)
    m = MaterialModel.from_arrays(sc, hdr, irrt, cf, albedo_res=ra, roughness_res=rr)
    m.lean_outputs = True                         # what the trainer sets
    with torch.no_grad():
        m.materials_a.copy_(a0.cuda())
        m.materials_r.copy_(r0.cuda())
    oracle = MS.MaterialStepOracle(osc, verts, tris, tri_uvs, cn, irrt, a0, r0, c, 16)
    oracle._gb = _OGB.setdefault((c, seed), {})
    views = {}
    for key, E in (("v0", cameras.grid_cameras(2)[0]), ("v1", cameras.grid_cameras(2)[3])):
        if key not in view_keys:
            continue
        mvp, cam = cameras.cube_mvps(E)
        gb = m._gbuffer(mvp, key)
        ogb = oracle.gbuffer(key, mvp.numpy())
        same = gb["tri_id"].reshape(-1).cpu().numpy() == ogb["tri_id"]
        gt = torch.rand(6, c, c, 3, generator=gen) * 1.5
        gmask = (torch.rand(6, c, c, 1, generator=gen) > 0.1).float()
        segs = torch.randint(40, 49, (6, c, c, 1), generator=gen).float()
        seg, fm, _ = build_masks(segs, torch.rand(6, c, c, 3, generator=gen) - 0.5)
        rooms = torch.randint(0, 2, (6, c, c, 1), generator=gen).float()
        room = ((torch.arange(2.0).reshape(2, 1, 1, 1, 1) - rooms.unsqueeze(0)) == 0).float()
        # pixels where ray casting and rasterisation pick different triangles (silhouette tie-breaks; their share is what tests/test_gpu_raster.py
        # measures) carry no class and no ground truth on BOTH sides: one such pixel is 1 / 6144 of the image and would alone cost 1e-2 of a gradient
        drop = torch.from_numpy(~same).reshape(6, c, c, 1)
        seg = seg * (~drop).float()
        fm = fm * (~drop).float()
        room = room * (~drop).float()
        gmask = gmask * (~drop).float()
        views[key] = dict(mvp=mvp, cam=cam, gt=gt, gmask=gmask, seg=seg, fm=fm, room=room, differ=int((~same).sum()))
    m._test_radiance_ratio = float(hdr.max() / np.median(hdr))           # lamp over base radiance (the edge scene: ~3600; the smooth scene: ~1.2)
    return m, oracle, views


def _deviating(got, ref, S=16, ratio=1.0):
    """the texels that `_rel_l2_but_few` sets aside, bounded one by one (VERDICT r5 next #3 / ADVICE r5): `count` = texels whose deviation exceeds 1e-3 of the LARGEST
    per-texel gradient, `worst` = the largest of THOSE deviations (0 when there is none) in units of what ONE specular sample crossing a lamp edge can add to a texel's
    gradient: the radiance jump (lamp over base = `ratio`) times one sample's weight (1 / S) times the rms per-texel gradient of the view's support"""
    d = (np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(-1, got.shape[-1])
    r = np.asarray(ref, np.float64).reshape(-1, got.shape[-1])
    dev, mag = np.sqrt((d ** 2).sum(-1)), np.sqrt((r ** 2).sum(-1))
    out = dev > 1e-3 * mag.max()
    unit = ratio / S * np.sqrt((mag[mag > 0] ** 2).mean())
    return int(out.sum()), (float(dev[out].max() / unit) if out.any() else 0.0)


def _rel_l2_but_few(got, ref, frac=5e-4, at_least=8):
    """relative L2 over all texels but the `max(at_least, frac * texels)` with the largest deviation.
    Why some texels are set aside: a specular sample is a ray, and the radiance a ray returns is discontinuous in its direction -- across the edge of an
    emissive rectangle it jumps by three orders of magnitude.  The product and the oracle evaluate the SAME estimator on G-buffers that agree to ~1e-5 in uv
    (ray casting vs rasterisation), so their fetched roughness differs by ~1e-5 and, once in a while, ONE of the 98 304 sample rays of a view lands on the
    other side of such an edge: that pixel's d rgb / d roughness differs by the jump, and with it the handful of texels under the pixel's taps -- at 128^2
    texels that handful carries 20 % of the gradient's norm.  Measured (round 5, profiles/r05/grad_edge_probe.txt): two builds of the product whose G-buffer uvs differ by
    one float32 ulp (fma contraction) give roughness gradients that differ in exactly 2 of 16 384 texels, by 1e-5, all parked mip stacks equal to 1e-12 -- and
    one build is 2e-5 from the oracle, the other 0.195.  Both are right; the comparison must not hinge on which side of an edge a ray falls."""
    d = (np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(-1, got.shape[-1])
    per = (d ** 2).sum(-1)
    k = max(at_least, int(frac * per.size))
    keep = np.argsort(per)[: per.size - k]
    r = np.asarray(ref, np.float64).reshape(-1, got.shape[-1])
    return float(np.sqrt(per[keep].sum()) / max(np.sqrt((r[keep] ** 2).sum()), 1e-30))


def _cu(v):
    return {k: (x.cuda() if torch.is_tensor(x) and k != "mvp" else x) for k, x in v.items()}


def _fresh_optimizer(m, stage):
    """trainer/train_material.py run(): fresh optimiser per stage, requires_grad toggles, clamps fused into the step"""
    from texir_code_amd.optim import FusedAdam
    if stage >= 1:
        m.materials_a.data = torch.clamp(m.materials_a.data, 0.0)
    m.materials_a.requires_grad = stage in (0, 2)
    m.materials_r.requires_grad = stage in (1, 2)
    opt = FusedAdam(m.parameters(), lr=LR, fuse_mip_fold=True)
    opt.set_clamp(m.materials_r, 1e-2, 0.8)
    if stage == 2:
        opt.set_clamp(m.materials_a, 0.0, float("inf"))
    return opt


@pytest.mark.parametrize("ra,rr", [(256, 512), (64, 128)])
def test_material_step_gradients_match_composite_torch_oracle(golden, ra, rr):
    """d loss / d materials_a and d loss / d materials_r of one eager step (FusedAdam.dense_grad: dense part + sparse level-0 part + parked
    level-1 / level-2 stacks folded down) against torch autograd through the oracle's own mip stack, stages 0 / 1 / 2, two views"""
    from texir_code_amd.loss import RenderLoss
    c = 32
    m, oracle, views = _world(golden, c, ra, rr)
    loss_fn = RenderLoss("L1", 1, lazy_item=True)
    gen = torch.Generator().manual_seed(3)
    worst, devs = {}, {}
    for stage in (0, 1, 2):
        opt = _fresh_optimizer(m, stage)
        oracle.make_optimizer(stage, LR)
        for key, v in views.items():
            assert v["differ"] <= 0.005 * 6 * c * c, v["differ"]
            shift = torch.rand(6 * c * c, 2, generator=gen)
            d = _cu(v)
            m._static_shift = shift.cuda()
            try:
                preds = m(v["mvp"], key, d["cam"], stage)
            finally:
                m._static_shift = None
            loss = loss_fn(d["gt"], preds, d["gmask"], d["fm"], d["seg"], stage=stage, room_seg_mask=d["room"] if stage == 2 else None)[0]
            opt.zero_grad()
            loss.backward()
            ga = opt.dense_grad(m.materials_a).cpu().numpy() if m.materials_a.requires_grad else None
            gr = opt.dense_grad(m.materials_r).cpu().numpy() if m.materials_r.requires_grad else None
            opt.zero_grad()
            lo, oa, orr = oracle.grads(key, v["mvp"].numpy(), v["cam"], stage, shift.numpy(), v["gt"], v["gmask"], v["fm"], v["seg"], v["room"])
            assert abs(float(loss.detach()) - lo) < 1e-4 * max(1.0, abs(lo)), (stage, key, float(loss.detach()), lo)
            for name, got, ref in (("a", ga, oa.numpy()), ("r", gr, orr.numpy())):
                if got is None:
                    continue
                assert np.abs(ref).max() > 0, (stage, key, name)
                e = _rel_l2_but_few(got, ref)
                worst[(stage, name)] = max(worst.get((stage, name), 0.0), e)
                assert e < 1e-3, (stage, key, name, e, rel_l2(got, ref))
                # the texels set aside are FEW and each one is at most what one edge-crossing sample can do (a localized bug -- an atlas border, a tap wrap, a seam --
                # moves dozens of texels by their own magnitude, or a few by more than a single sample's worth)
                count, worst_dev = _deviating(got, ref, 16, m._test_radiance_ratio)
                devs[(stage, name)] = (max(devs.get((stage, name), (0, 0.0))[0], count), max(devs.get((stage, name), (0, 0.0))[1], worst_dev))
                assert count <= 12 and worst_dev <= 1.0, (stage, key, name, count, worst_dev, rel_l2(got, ref))
                assert ((got != 0) == (ref != 0)).mean() > 0.99          # same support: the texels the view's taps touch
    print("composite material-step gradients vs torch oracle (%d^2 / %d^2 textures), worst rel-L2 per (stage, texture): %s; texels set aside (count, worst in single-sample units): %s"
          % (ra, rr, {k: "%.1e" % e for k, e in sorted(worst.items())}, {k: "%d, %.2g" % v for k, v in sorted(devs.items())}))
    # observed on MI355X (256^2 / 512^2): albedo 1e-5, roughness 1e-4 (stage 2) / 4e-4 (stage 1: d/d roughness of the GGX weights in float32 dual numbers
    # against float32 autograd, on lighting traced by two different tracers)
    assert max(worst.values()) < 6e-4


def _untrimmed_gradients(m, oracle, views, c, stages, bound, seed=3):
    """d loss / d materials of one eager step per (stage, view) against the oracle's autograd: PLAIN relative L2 over every texel, nothing set aside"""
    from texir_code_amd.loss import RenderLoss
    loss_fn = RenderLoss("L1", 1, lazy_item=True)
    gen = torch.Generator().manual_seed(seed)
    worst = {}
    for stage in stages:
        opt = _fresh_optimizer(m, stage)
        oracle.make_optimizer(stage, LR)
        for key, v in views.items():
            assert v["differ"] <= 0.005 * 6 * c * c, v["differ"]
            shift = torch.rand(6 * c * c, 2, generator=gen)
            d = _cu(v)
            m._static_shift = shift.cuda()
            try:
                preds = m(v["mvp"], key, d["cam"], stage)
            finally:
                m._static_shift = None
            loss = loss_fn(d["gt"], preds, d["gmask"], d["fm"], d["seg"], stage=stage, room_seg_mask=d["room"] if stage == 2 else None)[0]
            opt.zero_grad()
            loss.backward()
            ga = opt.dense_grad(m.materials_a).cpu().numpy() if m.materials_a.requires_grad else None
            gr = opt.dense_grad(m.materials_r).cpu().numpy() if m.materials_r.requires_grad else None
            opt.zero_grad()
            lo, oa, orr = oracle.grads(key, v["mvp"].numpy(), v["cam"], stage, shift.numpy(), v["gt"], v["gmask"], v["fm"], v["seg"], v["room"])
            assert abs(float(loss.detach()) - lo) < 1e-4 * max(1.0, abs(lo)), (stage, key, float(loss.detach()), lo)
            for name, got, ref in (("a", ga, oa.numpy()), ("r", gr, orr.numpy())):
                if got is None:
                    continue
                assert np.abs(ref).max() > 0, (stage, key, name)
                e = rel_l2(got, ref)
                worst[(stage, name)] = max(worst.get((stage, name), 0.0), e)
                assert e < bound, (stage, key, name, e)                     # north_star: material-step grads within 1e-3, every texel counted
                assert ((got != 0) == (ref != 0)).mean() > 0.99
    return worst


@pytest.mark.parametrize("ra,rr", [(256, 512), (64, 128)])
def test_material_step_gradients_untrimmed_on_smooth_radiance(golden, ra, rr):
    """the same composite step on a scene whose radiance texture has no step edges -- plain rel-L2 < 1e-3 on d albedo / d roughness for stages
    0 / 1 / 2, both views, with NO texel set aside (mat_nvdiffrast.py:131-139,234-241; loss.py:81-115)"""
    c = 32
    m, oracle, views = _world(golden, c, ra, rr, smooth=True)
    assert m._test_radiance_ratio < 1.5
    worst = _untrimmed_gradients(m, oracle, views, c, (0, 1, 2), 1e-3)
    print("composite material-step gradients vs torch oracle, smooth radiance, UNTRIMMED (%d^2 / %d^2 textures): %s" % (ra, rr, {k: "%.1e" % e for k, e in sorted(worst.items())}))


def test_material_step_gradients_untrimmed_at_4k_textures(golden):
    """the composite oracle at the C3 texture size (BASELINE.json configs[2]: 4096^2 albedo / roughness; the torch oracle's mip stacks are ~270 + 90 MB): one 6 x 32^2 view,
    stages 1 and 2, plain rel-L2 over all 16.8 M texels.  At this size a pixel's footprint spans ~2^5 texels: the taps sit on mip levels 4-6 and the level-0
    gradient is what the deferred folds spread out of them -- the part of the backward no smaller oracle run exercises"""
    c = 32
    m, oracle, views = _world(golden, c, 4096, 4096, smooth=True, view_keys=("v0",))
    worst = _untrimmed_gradients(m, oracle, views, c, (1, 2), 1e-3)
    print("composite material-step gradients vs torch oracle at 4096^2 / 4096^2 textures, UNTRIMMED: %s" % {k: "%.1e" % e for k, e in sorted(worst.items())})


@pytest.mark.parametrize("ra,rr", [(256, 512), (64, 128)])
def test_material_step_trajectory_through_hipgraph_matches_composite_torch_oracle(golden, ra, rr):
    """the trainer's three stages, three optimiser steps each (views v0, v1, v0), every step ONE hipGraph replay containing forward, loss,
    backward and the fused Adam step: textures after every stage against torch.optim.Adam on the oracle's autograd gradients"""
    from texir_code_amd.graph_step import GraphedMatStep
    from texir_code_amd.loss import RenderLoss
    c = 32
    m, oracle, views = _world(golden, c, ra, rr)
    loss_fn = RenderLoss("L1", 1, lazy_item=True, unit_upstream=True)
    gen = torch.Generator().manual_seed(4)
    dv = {k: _cu(v) for k, v in views.items()}
    for stage in (0, 1, 2):
        opt = _fresh_optimizer(m, stage)
        oracle.make_optimizer(stage, LR)
        if stage >= 1:
            with torch.no_grad():
                oracle.a.clamp_(min=0.0)                                     # train_material.py:477
        gs = GraphedMatStep(m, loss_fn, opt, [m.materials_a, m.materials_r])
        for key, d in dv.items():
            gs.capture(key, views[key]["mvp"], d["cam"], d["gt"], d["gmask"], d["seg"], d["fm"], d["room"] if stage == 2 else None, stage)
        assert gs.step_in_graph
        for key in ("v0", "v1", "v0"):
            v = views[key]
            shift = torch.rand(6 * c * c, 2, generator=gen)
            loss = gs.step(key, stage, shift=shift)
            lo = oracle.step(key, v["mvp"].numpy(), v["cam"], stage, shift.numpy(), v["gt"], v["gmask"], v["fm"], v["seg"], v["room"])
            assert abs(float(loss) - lo) < 2e-4 * max(1.0, abs(lo)), (stage, key, float(loss), lo)
        for name, got, ref in (("a", m.materials_a, oracle.a), ("r", m.materials_r, oracle.r)):
            got, ref = got.detach().cpu().numpy(), ref.detach().numpy()
            # Adam's first steps move a texel by ~lr whatever the size of its gradient: a texel whose gradient is a rounding-level residue (|g| ~ eps)
            # may legitimately go the other way.  Everything else must agree to float precision.
            close = np.abs(got - ref) < 1e-4
            assert close.mean() > 0.999, (stage, name, close.mean())
            e = rel_l2(got[close], ref[close])
            print("stage %d texture %s after 3 graph steps: %.4f %% of texels within 1e-4, rel-L2 of those %.1e (all: %.1e)"
                  % (stage, name, 100 * close.mean(), e, rel_l2(got, ref)))
            assert e < 1e-5, (stage, name, e)
            assert rel_l2(got, ref) < 1e-3, (stage, name, rel_l2(got, ref))
    # the stages moved what they should
    assert float((m.materials_a.detach().cpu() - oracle.a.detach()).abs().max()) < 0.2
