"""Cases of the multi-texture IrT pass (include/texir_hip.h texir_irt_multi, csrc/irtmulti.hip): the textures, the listed texels, the float64 reference of
one texture and a float32 restatement of the rule with the mutants its check must reject.  Shared by test_irt_multi_ref_cpu.py (no GPU) and
test_gpu_irt_multi.py (no tests here).  Everything about rays, intervals and caps comes from trace_cases, which is imported and not changed.

THE REFERENCE OF TEXTURE T is trace_cases.IrtRef on the scene whose texture is T: float64 brute force over all triangles with the intervals trace_cases
derives; nothing of the code under test enters it.  out[k] must lie inside the intervals of T_k in the 64-texel form ('group', n_parts(N, 'group')), and
-- the sharper statement, device against device -- equal irt_generate after set_texture(T_k) bit for bit.
"""
import numpy as np

import trace_cases as TC

F32 = np.float32
SCENE = "room"
# listed texels: two full waves plus two lanes, one full wave, one wave plus one lane, one lane
LISTS = (130, 64, 65, 1)
N_EQUAL = (1, 64, 65, 100, 128, 512)
K_EQUAL = (1, 2, 3, 4, 5, 8)                        # every KMAX (2, 4, 8) and every K < KMAX
REF_TEXTURES = ("ramp", "random", "checker")
# (texture, listed texels, N) of the interval test; test_irt_multi_ref_cpu.py asserts the caps of every reference they need
REF_CASES = [(name, n_tex, N) for name in REF_TEXTURES for n_tex, N in ((130, 64), (70, 512))]
CPU_CASE = (10, 64)

_TEX = {}


def texture(name):
    """float32 [H,W,3] in the orientation of the scene's texture (H = W = 256 on the golden room)"""
    if name not in _TEX:
        geo, _ = TC.golden_geo(SCENE)
        H, W = geo.hdr.shape[:2]
        x = np.arange(W, dtype=F32)[None, :] + np.zeros((H, 1), F32)
        y = np.arange(H, dtype=F32)[:, None] + np.zeros((1, W), F32)
        if name == "ramp":
            t = np.stack([F32(0.1) + x / F32(W), F32(0.1) + y / F32(H), F32(0.6) + F32(0.4) * np.sin(x / F32(9)) * np.cos(y / F32(7))], -1)
        elif name == "random":
            t = np.random.default_rng(31).random((H, W, 3))
        elif name == "checker":
            t = np.repeat((((x // 8 + y // 8) % 2))[..., None], 3, -1)
        elif name == "hdr":
            t = geo.hdr
        elif name == "lamp":
            from texir_code_amd import irtsplit
            t = geo.hdr * (irtsplit.labels_from_radiance(geo.hdr, 0.0) == 1)[..., None]
        elif name == "ones":
            t = np.ones((H, W, 3), F32)
        elif name == "special":
            # NaN, Inf and a negative value among ordinary ones: nothing but the same multiplications and additions
            t = texture("random").copy()
            t[::5, ::7, 0], t[1::9, 2::4, 1], t[::3, 1::2, 2] = np.nan, np.inf, -2.5
        else:
            raise KeyError(name)
        _TEX[name] = np.ascontiguousarray(t, F32)
        _TEX[name].setflags(write=False)
    return _TEX[name]


def textures(names):
    """[K,H,W,3]"""
    return np.ascontiguousarray(np.stack([texture(n) for n in names]))


# K textures for the equality tests: the three of the interval test, the room's own, its lamps and repeats under other scales
def k_textures(K):
    base = ("ramp", "random", "checker", "hdr", "lamp")
    out = [texture(base[k % len(base)]) * F32(1 + k // len(base)) for k in range(K)]
    return np.ascontiguousarray(np.stack(out), F32)


def tex_geo(tex, tag):
    geo, _ = TC.golden_geo(SCENE)
    return TC.Geo("%s_%s" % (SCENE, tag), geo.verts, geo.tris, geo.tri_uvs, np.ascontiguousarray(tex, F32))


_REF = {}


def multi_ref(name, n_tex, N):
    """IrtRef of texture `name` on the listed texels of irt_case(room, n_tex, N): computed once, shared, never changed"""
    key = (name, n_tex, N)
    if key not in _REF:
        c = TC.irt_case(SCENE, n_tex, N, "uniform")
        i = c.ids
        _REF[key] = TC.IrtRef(tex_geo(texture(name), name), c.pos[i], c.nrm[i], c.shift[i], N, "uniform")
    return _REF[key]


# ---- float32 restatement --------------------------------------------------------------------------------------------------------------------------------

MUTANTS = ("swapped", "rows_reversed", "transposed", "bgr", "planar", "leak")


def traced(n_tex, N):
    """float32 brute-force hits of the case's samples: (case, dirs [P,N,3], t, pid, uv)"""
    from oracle import oracle as O
    c = TC.irt_case(SCENE, n_tex, N, "uniform")
    i = c.ids
    d = O.generate_dir(c.nrm[i], N, c.mode, c.shift[i])
    t, pid, uv = TC.trace_f32(c.geo, np.repeat(c.pos[i], N, 0), d.reshape(-1, 3))
    return c, d, t, pid, uv


def multi_f32(case, d, t, pid, uv, tex, mut=None):
    """the rule in float32, op by op: trace_f32's hits, shade_f32 on T_k read out of the interleaved buffer [H,W,K,3], estimator_f32 in the 64-texel form
    -> [K,P,3].  tex [K,H,W,3].  mut: 'swapped' (textures k and k + 1 change places) | 'rows_reversed' | 'transposed' | 'bgr' | 'planar' (the interleaved
    buffer indexed as [K,H,W,3]) | 'leak' (k = 0 reads the scene's own texture)"""
    i, N = case.ids, case.N
    parts = TC.n_parts(N, "group")
    K, H, W, _ = tex.shape
    buf = np.ascontiguousarray(tex.transpose(1, 2, 0, 3))                    # what the kernel is handed
    out = np.zeros((K, len(i), 3), F32)
    for k in range(K):
        q = k ^ 1 if (mut == "swapped" and (k ^ 1) < K) else k
        T = buf.reshape(K, H, W, 3)[q] if mut == "planar" else buf[:, :, q, :]
        if mut == "rows_reversed":
            T = T[::-1]
        elif mut == "transposed":
            T = T.transpose(1, 0, 2)
        elif mut == "bgr":
            T = T[..., ::-1]
        elif mut == "leak" and k == 0:
            T = case.geo.hdr
        L = TC.shade_f32(tex_geo(T, "f32"), t, pid, uv)
        out[k] = TC.estimator_f32(case.nrm[i], d, L.reshape(len(i), N, 3), False, "group", parts)
    return out


# ---- a stub scene for the helpers of irtlight.py: records the textures it is handed, answers with a fixed linear map -----------------------------------------

class StubScene:
    """irt_multi(textures [K,Ht,Wt,3]) -> [K,Nt,3]: every point's value is gain * the mean of its texture, so that bounce's compositions can be restated"""

    def __init__(self, tex_hw, gain=0.5):
        self.tex_shape = (int(tex_hw[0]), int(tex_hw[1]), 3)
        self.gain = gain
        self.calls = []

    def irt_multi(self, pos, nrm, shift, n_samples, textures, mode="uniform", texel_ids=None, out=None, **kw):
        import torch
        t = torch.as_tensor(textures)
        assert tuple(t.shape[1:]) == self.tex_shape and t.dtype == torch.float32 and t.is_contiguous()
        self.calls.append(dict(textures=t.clone(), n_samples=n_samples, texel_ids=texel_ids))
        Nt = pos.shape[0]
        m = t.reshape(t.shape[0], -1, 3).mean(1) * self.gain                      # [K,3]
        w = torch.linspace(0.5, 1.5, Nt, dtype=torch.float32)
        return (m[:, None, :] * w[None, :, None]).contiguous()
