"""RenderLoss's cache of compacted mask ids (texir_code_amd/loss.py RenderLoss._compact) -- host-only, no GPU.

The cache is keyed by (data_ptr, shape, _version) of the mask tensors.  A mask that is freed and replaced by a new one of the same shape
can land at the same address with the same _version; the cache must then compute the new mask's ids instead of serving the old ones."""
import gc
import weakref

import numpy as np
import torch

from texir_code_amd.loss import NO_CLASS, RenderLoss


def _onehot(ids, C):
    """[F,h,w] class ids (NO_CLASS = no class) -> [C,F,h,w,1] float32 one-hot mask"""
    return (np.arange(C).reshape(C, 1, 1, 1) == ids[None]).astype(np.float32)[..., None]


def test_fresh_mask_at_a_reused_address_gets_its_own_ids():
    """a numpy buffer refilled with a new mask and wrapped by a new tensor each time: same address, shape and _version every call"""
    C, F, h, w = 5, 6, 4, 4
    rng = np.random.default_rng(0)
    L = RenderLoss("L1")
    arr = np.zeros((C, F, h, w, 1), np.float32)
    fm_arr = np.zeros_like(arr)
    for _ in range(20):
        ids = rng.integers(0, C, (F, h, w))
        ids[0, 0, :2] = NO_CLASS
        hl = rng.random((F, h, w)) > 0.5
        arr[:] = _onehot(ids, C)
        fm_arr[:] = arr * hl[None, ..., None]
        seg, fm = torch.from_numpy(arr), torch.from_numpy(fm_arr)
        seg_id, hl_id, room_id, c, r = L._compact(seg, fm, None, "cpu")
        assert torch.equal(seg_id, torch.from_numpy(ids.reshape(-1).astype(np.uint8)))
        assert torch.equal(hl_id, torch.from_numpy((hl & (ids != NO_CLASS)).reshape(-1).astype(np.uint8)))
        assert room_id is None and (c, r) == (C, 0)
        del seg, fm


def test_live_mask_hits_and_an_inplace_change_misses():
    C = 3
    rng = np.random.default_rng(1)
    L = RenderLoss("L1")
    ids = rng.integers(0, C, (6, 2, 3))
    seg = torch.from_numpy(_onehot(ids, C))
    room = torch.from_numpy(_onehot(rng.integers(0, 2, (6, 2, 3)), 2))
    first = L._compact(seg, None, room, "cpu")
    assert L._compact(seg, None, room, "cpu") is first            # same live tensors, unchanged: the cached ids themselves
    seg.zero_()
    seg[1] = 1.0                                                   # every pixel now class 1: the version bump forces a recompute
    got = L._compact(seg, None, room, "cpu")
    assert got is not first and bool((got[0] == 1).all())
    assert torch.equal(got[2], first[2])


def test_cache_does_not_keep_masks_alive():
    C = 4
    L = RenderLoss("L2")
    seg = torch.from_numpy(_onehot(np.random.default_rng(2).integers(0, C, (6, 3, 3)), C))
    ref = weakref.ref(seg)
    L._compact(seg, None, None, "cpu")
    del seg
    gc.collect()
    assert ref() is None
    # the dead entry is dropped by the next miss
    L._compact(torch.from_numpy(_onehot(np.zeros((6, 3, 3), np.int64), C)), None, None, "cpu")
    assert len(L._cache) == 1
