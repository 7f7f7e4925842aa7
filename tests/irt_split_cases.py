"""Cases of the irradiance split by source label (include/texir_hip.h texir_irt_split, csrc/irtsplit.hip): the label images, the listed texels, the float64
reference of one class and a float32 restatement of the rule with the mutants its check must reject.  Shared by test_irt_split_ref_cpu.py (no GPU) and
test_gpu_irt_split.py (no tests here).  Everything about rays, intervals and caps comes from trace_cases, which is imported and not changed.

THE REFERENCE OF CLASS k is trace_cases.IrtRef on the scene whose texture is hdr * [label == k]: float64 brute force over all triangles with the
intervals trace_cases derives; nothing of the code under test enters it.  The split's out[k] must lie inside its intervals in the 64-texel form
('group', n_parts(N, 'group')), and -- the sharper statement, device against device -- equal irt_generate on that masked texture bit for bit.
"""
import numpy as np

import trace_cases as TC

F32 = np.float32
SCENE = "room"
# listed texels: two full waves plus two lanes, one full wave, one wave plus one lane, one lane
LISTS = (130, 64, 65, 1)
N_EQUAL = (1, 64, 65, 100, 128, 512)
# (label image, listed texels, N) of the interval test; test_irt_split_ref_cpu.py asserts the caps of every reference they need
REF_CASES = [(name, n_tex, N) for name in ("lamp", "bands") for n_tex, N in ((130, 64), (70, 512))]
CPU_CASE = (10, 64)

_LABELS = {}


def labels(name):
    """(K, uint8 [H,W] in the orientation of the scene's texture)"""
    if name not in _LABELS:
        from texir_code_amd import irtsplit
        geo, _ = TC.golden_geo(SCENE)
        H, W = geo.hdr.shape[:2]
        rows = (np.arange(H)[:, None] * 3 // H + np.zeros((1, W), np.int64)).astype(np.uint8)
        if name == "lamp":
            v = (2, irtsplit.labels_from_radiance(geo.hdr, 0.0))
        elif name == "bands":
            v = (3, rows)
        elif name == "random8":
            v = (8, np.random.default_rng(20).integers(0, 8, (H, W)).astype(np.uint8))
        elif name == "zeros":
            v = (1, np.zeros((H, W), np.uint8))
        elif name == "dropped":
            v = (2, rows)                                                      # class 2 of `bands` belongs to nobody
        else:
            raise KeyError(name)
        _LABELS[name] = (v[0], np.ascontiguousarray(v[1]))
    return _LABELS[name]


LABEL_NAMES = ("lamp", "bands", "random8", "zeros", "dropped")


def masked_hdr(lab, k, hdr=None, unit=False):
    """the texture of class k: hdr * [label == k] (unit: the indicator texture)"""
    geo, _ = TC.golden_geo(SCENE)
    m = (lab == k)[..., None]
    if unit:
        return np.ascontiguousarray(np.broadcast_to(m, m.shape[:2] + (3,)).astype(F32))
    return np.ascontiguousarray((geo.hdr if hdr is None else hdr) * m).astype(F32)


def masked_geo(lab, k, tag=""):
    geo, _ = TC.golden_geo(SCENE)
    return TC.Geo("%s_%s%d" % (SCENE, tag, k), geo.verts, geo.tris, geo.tri_uvs, masked_hdr(lab, k))


_REF = {}


def split_ref(name, k, n_tex, N):
    """IrtRef of class k of label image `name` on the listed texels of irt_case(room, n_tex, N): computed once, shared, never changed"""
    key = (name, k, n_tex, N)
    if key not in _REF:
        c = TC.irt_case(SCENE, n_tex, N, "uniform")
        i = c.ids
        _REF[key] = TC.IrtRef(masked_geo(labels(name)[1], k, name), c.pos[i], c.nrm[i], c.shift[i], N, "uniform")
    return _REF[key]


# ---- float32 restatement --------------------------------------------------------------------------------------------------------------------------------

MUTANTS = ("nearest_label", "flipped", "transposed", "off_by_one", "folded")
# the label image a mutant is tried on: one it changes the split of
MUTANT_LABELS = {"nearest_label": "random8", "flipped": "lamp", "transposed": "bands", "off_by_one": "bands", "folded": "dropped"}


def traced(n_tex, N):
    """float32 brute-force hits of the case's samples: (case, dirs [P,N,3], t, pid, uv)"""
    from oracle import oracle as O
    c = TC.irt_case(SCENE, n_tex, N, "uniform")
    i = c.ids
    d = O.generate_dir(c.nrm[i], N, c.mode, c.shift[i])
    t, pid, uv = TC.trace_f32(c.geo, np.repeat(c.pos[i], N, 0), d.reshape(-1, 3))
    return c, d, t, pid, uv


def split_f32(case, d, t, pid, uv, lab, K, mut=None):
    """the rule in float32, op by op: trace_f32's hits, shade_f32 on the texture hdr * [label == k], estimator_f32 in the 64-texel form -> [K,P,3].
    mut: 'nearest_label' (one label for the whole footprint, the nearest texel's) | 'flipped' (labels upside down) | 'transposed' |
    'off_by_one' (out[k] holds class k + 1) | 'folded' (labels >= K count as class K - 1)"""
    i, N = case.ids, case.N
    parts = TC.n_parts(N, "group")
    H, W = lab.shape
    if mut == "flipped":
        lab = lab[::-1]
    elif mut == "transposed":
        lab = np.ascontiguousarray(lab.T)
    elif mut == "folded":
        lab = np.minimum(lab, K - 1)
    near = None
    if mut == "nearest_label":
        # where the footprint lies: the bilinear fetch of an image of texel coordinates is the sample position (to a rounding far below half a texel)
        xy = np.zeros((H, W, 3), F32)
        xy[..., 0], xy[..., 1] = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
        g = TC.Geo("xy", case.geo.verts, case.geo.tris, case.geo.tri_uvs, xy)
        p = TC.shade_f32(g, t, pid, uv)
        near = lab[np.clip(np.rint(p[:, 1]), 0, H - 1).astype(np.int64), np.clip(np.rint(p[:, 0]), 0, W - 1).astype(np.int64)]
        full = TC.shade_f32(case.geo, t, pid, uv)
    out = np.zeros((K, len(i), 3), F32)
    for k in range(K):
        cls = (k + 1) % max(K, 2) if mut == "off_by_one" else k
        if near is not None:
            L = np.where((near == cls)[:, None], full, F32(0)).astype(F32)
        else:
            L = TC.shade_f32(masked_geo(lab, cls, "f32"), t, pid, uv)
        out[k] = TC.estimator_f32(case.nrm[i], d, L.reshape(len(i), N, 3), False, "group", parts)
    return out
