"""irt_multi_kernel (csrc/irtmulti.hip) and irt_combine_kernel (csrc/kernels.hip) behind texir_irt_multi, Scene.irt_multi, irtlight.bounce, the IrT stage's
train.irt_light_bounces, `light-irt --bounce` and the evaluation model's test.light_bounces, on the golden room (20 k triangles, 256^2 texture).

  1. intervals     every texture of (ramp, random, checker) inside the float64 reference of the scene that holds it (irt_multi_cases.multi_ref);
  2. equality      bit for bit the existing 64-texel kernel after set_texture(T_k): K in 1, 2, 3, 4, 5, 8, N in 1, 64, 65, 100, 128, 512 and once 2048, lists
                   of 130 / 64 / 65 / 1 texels; two parts and one part under TEXIR_IRT_MIN_PART_CELLS / TEXIR_IRT_LOG2PARTS; NaN, Inf and negative texels;
                   an RGBE-born scene (layout 4); the masked textures of irt_split;
  3. independence  NaN in texture j changes no bit of out[k != j];
  4. purity        shuffled list, three slices, second run, side stream, a captured graph replayed twice and once more on overwritten textures: identical
                   bits; sentinels and guard words intact;
  5. errors        every refused argument raises;
  6. bounce        irtlight.bounce is the composition it documents; the orientation pin; the energy ceiling; the stage and the command; the evaluation model.
"""
import json
import os

import numpy as np
import pytest
import torch

import irt_multi_cases as MC
import irt_split_cases as SP
import trace_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GROUP = "irt_group_kernel<false, 4, 6>"
_SC = {}


def world(tx, kind="float"):
    """(scene holding the room's own texture, scene whose texture set_texture replaces, the room's texture) -- kind 'float' | 'born'"""
    if kind not in _SC:
        from texir_code_amd import synth
        geo, _ = TC.golden_geo(MC.SCENE)
        hdr = geo.hdr if kind == "float" else synth.rgbe_born(geo.hdr)
        full, other = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, hdr), tx.Scene(geo.verts, geo.tris, geo.tri_uvs, hdr)
        assert full.texture_layout() == (2 if kind == "float" else 4)
        _SC[kind] = (full, other, np.ascontiguousarray(hdr, np.float32))
    return _SC[kind]


_DEV = {}


def texel_inputs():
    if not _DEV:
        c = TC.irt_case(MC.SCENE, 130, 64, "uniform")
        _DEV["v"] = tuple(torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.shift))
    return _DEV["v"]


def ids_of(n):
    return torch.from_numpy(TC.listed(MC.SCENE, n).astype(np.int32)).cuda()


def multi(sc, tex, N, ids, **kw):
    pos, nrm, shift = texel_inputs()
    K = tex.shape[2] if kw.get("interleaved") else tex.shape[0]
    out = torch.full((K, pos.shape[0], 3), SENTINEL, device="cuda")
    got = sc.irt_multi(pos, nrm, shift, N, tex if torch.is_tensor(tex) else torch.from_numpy(tex), texel_ids=ids, out=out, **kw)
    assert got is out
    return out.cpu().numpy()


def generate(sc, N, ids):
    pos, nrm, shift = texel_inputs()
    out = torch.full((pos.shape[0], 3), SENTINEL, device="cuda")
    return sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, out=out).cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def assert_same_bits(g, want, what):
    if not same_bits(g, want):
        bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d values differ; first at %s: irt_multi %r, set_texture + irt_generate %r"
                             % (what, len(bad), bad[0], float(g[tuple(bad[0])]), float(want[tuple(bad[0])])))


# ---- 1. intervals ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tex,N", [(130, 64), (70, 512)])
def test_every_texture_inside_the_float64_reference_of_its_scene(tx, n_tex, N):
    full, _, _ = world(tx)
    use = TC.listed(MC.SCENE, n_tex)
    got = multi(full, MC.textures(MC.REF_TEXTURES), N, ids_of(n_tex))
    parts = TC.n_parts(N, "group")
    for k, name in enumerate(MC.REF_TEXTURES):
        worst = MC.multi_ref(name, n_tex, N).check(got[k][use], "group", parts, "irt_multi", "%s %dx%d" % (name, n_tex, N))
        print("irt_multi %s %dx%d: worst share of the interval %.3f" % (name, n_tex, N, worst))
    unlisted = np.ones(got.shape[1], bool)
    unlisted[use] = False
    assert (got[:, unlisted] == SENTINEL).all()


# ---- 2. equality with the existing kernel ----------------------------------------------------------------------------------------------------------------------

_WANT = {}


def want_of(tx, key, T, Ns, lists, env=""):
    """irt_generate in its 64-texel form on the second scene after set_texture(T): computed once per (texture, switches), shared"""
    _, other, _ = world(tx)
    missing = [(N, n) for N in Ns for n in lists if (key, env, N, n) not in _WANT]
    if missing:
        other.set_texture(np.ascontiguousarray(T, np.float32))
        for N, n in missing:
            assert other.irt_kernel_name(n, N) == GROUP
            _WANT[(key, env, N, n)] = generate(other, N, ids_of(n))
    return {(N, n): _WANT[(key, env, N, n)] for N in Ns for n in lists}


@pytest.mark.parametrize("K", MC.K_EQUAL)
def test_multi_equals_the_64_texel_kernel_after_set_texture(tx, monkeypatch, K):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    full, _, _ = world(tx)
    tex = MC.k_textures(K)
    got = {(N, n): multi(full, tex, N, ids_of(n)) for N in MC.N_EQUAL for n in MC.LISTS}
    for k in range(K):
        want = want_of(tx, "k%d" % k, tex[k], MC.N_EQUAL, MC.LISTS)
        for (N, n), w in want.items():
            assert_same_bits(got[(N, n)][k], w, "K=%d texture %d N=%d list=%d" % (K, k, N, n))


def test_multi_equals_the_set_texture_runs_at_2048_samples(tx, monkeypatch):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    full, _, _ = world(tx)
    tex = MC.k_textures(3)
    got = multi(full, tex, 2048, ids_of(130))
    for k in range(3):
        assert_same_bits(got[k], want_of(tx, "k%d" % k, tex[k], (2048,), (130,))[(2048, 130)], "texture %d N=2048" % k)


@pytest.mark.parametrize("N,switch,value,parts", [(128, "TEXIR_IRT_MIN_PART_CELLS", "64", 2), (64, "TEXIR_IRT_LOG2PARTS", "0", 1)])
def test_multi_equals_the_64_texel_kernel_under_the_switches_of_the_plan(tx, monkeypatch, N, switch, value, parts):
    from texir_code_amd import _lib
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    monkeypatch.setenv(switch, value)
    assert int(_lib.lib().texir_irt_multi_workspace_bytes(1, N, 3)) == 12 * 3 * parts
    full, _, _ = world(tx)
    tex = MC.k_textures(3)
    got = multi(full, tex, N, ids_of(130))
    for k in range(3):
        assert_same_bits(got[k], want_of(tx, "k%d" % k, tex[k], (N,), (130,), env=switch + value)[(N, 130)], "texture %d N=%d %s=%s" % (k, N, switch, value))


def test_nan_inf_and_negative_texels_are_the_same_bits_too(tx, monkeypatch):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    full, _, _ = world(tx)
    tex = MC.textures(("special", "ramp"))
    for N, n in ((128, 130), (100, 65)):
        got = multi(full, tex, N, ids_of(n))
        use = TC.listed(MC.SCENE, n)
        assert np.isnan(got[0][use]).any() and np.isfinite(got[1][use]).all()
        for k, name in enumerate(("special", "ramp")):
            assert_same_bits(got[k], want_of(tx, name, tex[k], (N,), (n,))[(N, n)], "%s N=%d list=%d" % (name, N, n))


def test_on_an_rgbe_born_scene_copies_of_its_texture_equal_its_untouched_irt_generate(tx, monkeypatch):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    born, _, hdr = world(tx, "born")
    tex = np.ascontiguousarray(np.stack([hdr] * 3))
    for N, n in ((64, 130), (100, 65), (512, 64)):
        assert born.irt_kernel_name(n, N) == GROUP and born.texture_layout() == 4
        got, want = multi(born, tex, N, ids_of(n)), generate(born, N, ids_of(n))
        for k in range(3):
            assert_same_bits(got[k], want, "born copy %d N=%d list=%d" % (k, N, n))


def test_masked_textures_equal_irt_split(tx):
    K, lab = SP.labels("bands")
    full, _, hdr = world(tx)
    tex = np.ascontiguousarray(np.stack([SP.masked_hdr(lab, k, hdr) for k in range(K)]))
    pos, nrm, shift = texel_inputs()
    for N, n in ((64, 130), (100, 65), (512, 64)):
        out = torch.full((K, pos.shape[0], 3), SENTINEL, device="cuda")
        full.irt_split(pos, nrm, shift, N, torch.from_numpy(lab), K, texel_ids=ids_of(n), out=out)
        assert_same_bits(multi(full, tex, N, ids_of(n)), out.cpu().numpy(), "bands N=%d list=%d" % (N, n))


# ---- 3. independence ----------------------------------------------------------------------------------------------------------------------------------------------

def test_nan_in_one_texture_changes_no_bit_of_the_others(tx):
    full, _, _ = world(tx)
    for K in (2, 4, 8):
        tex = MC.k_textures(K)
        base = multi(full, tex, 128, ids_of(130))
        for j in (0, K - 1):
            poisoned = tex.copy()
            poisoned[j] = np.nan
            got = multi(full, poisoned, 128, ids_of(130))
            use = TC.listed(MC.SCENE, 130)
            assert np.isnan(got[j][use]).any()
            for k in range(K):
                if k != j:
                    assert same_bits(got[k], base[k]), (K, j, k)


# ---- 4. purity -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_result_is_a_pure_function_of_the_inputs(tx):
    from texir_code_amd import _lib
    K = 5
    tex = MC.k_textures(K)
    full, _, _ = world(tx)
    N, n = 128, 130
    ids, use = ids_of(n), TC.listed(MC.SCENE, n)
    base = multi(full, tex, N, ids)
    unlisted = np.ones(base.shape[1], bool)
    unlisted[use] = False
    assert (base[:, unlisted] == SENTINEL).all() and np.isfinite(base).all() and (base[:, use] != SENTINEL).all()
    assert np.array_equal(base, multi(full, tex, N, ids)), "second run"
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    assert np.array_equal(base, multi(full, tex, N, ids[perm])), "shuffled list"
    L = _lib.lib()
    per_texel = int(L.texir_irt_multi_workspace_bytes(1, N, K))
    assert per_texel == 12 * K * TC.n_parts(N, "group")
    assert np.array_equal(base, multi(full, tex, N, ids, max_workspace_bytes=64 * per_texel)), "three slices (64 + 64 + 2 texels)"
    # the interleaved form in place of the friendly one
    inter = torch.from_numpy(tex).cuda().permute(1, 2, 0, 3).contiguous()
    assert np.array_equal(base, multi(full, inter, N, ids, interleaved=True)), "interleaved=True"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = multi(full, tex, N, ids)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(base, on_side), "side stream"
    # a captured graph on caller-owned buffers with guard words behind `out` and behind the workspace: replayed twice, then once more after the
    # textures were overwritten on the device -- a replay reads whatever tex holds then
    pos, nrm, shift = texel_inputs()
    Nt, guard = pos.shape[0], 64
    out = torch.full((K * Nt * 3 + guard,), SENTINEL, device="cuda")
    need = int(L.texir_irt_multi_workspace_bytes(n, N, K))
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.texir_irt_multi(full.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n, Nt, N, 0, _lib.ptr(inter), K, _lib.ptr(out),
                                         _lib.ptr(ws), need, _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)

    def replay(want, what):
        out.fill_(SENTINEL)
        ws[:need].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(want, out[:K * Nt * 3].reshape(K, Nt, 3).cpu().numpy()), what
        assert (out[K * Nt * 3:] == SENTINEL).all() and (ws[need:] == 0xA5).all(), "guard words"
    replay(base, "graph replay")
    replay(base, "second graph replay")
    other = np.ascontiguousarray(tex[::-1] * np.float32(0.5) + np.float32(0.25))
    inter.copy_(torch.from_numpy(other).cuda().permute(1, 2, 0, 3))
    eager = multi(full, other, N, ids)
    assert not np.array_equal(eager, base)
    replay(eager, "graph replay on overwritten textures")


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise(tx, monkeypatch):
    from texir_code_amd import _lib
    K = 3
    tex = torch.from_numpy(MC.k_textures(K))
    full, _, _ = world(tx)
    H, W = full.tex_shape[:2]
    pos, nrm, shift = texel_inputs()
    ids = ids_of(65)
    for bad_k in (0, 9):
        with pytest.raises(_lib.TexirError, match="K must be in 1..8, got %d" % bad_k):
            full.irt_multi(pos, nrm, shift, 64, torch.zeros((bad_k, H, W, 3)), texel_ids=ids)
    for bad_n in (0, -64):
        with pytest.raises(_lib.TexirError, match="bad sizes"):
            full.irt_multi(pos, nrm, shift, bad_n, tex, texel_ids=ids)
    for bad in (tex[0], tex[:, :-1], tex[..., :2], tex.permute(1, 2, 0, 3)):
        with pytest.raises(ValueError, match="textures must be"):
            full.irt_multi(pos, nrm, shift, 64, bad, texel_ids=ids)
    with pytest.raises(ValueError, match="textures must be"):
        full.irt_multi(pos, nrm, shift, 64, tex, texel_ids=ids, interleaved=True)
    with pytest.raises(ValueError, match="out must be"):
        full.irt_multi(pos, nrm, shift, 64, tex, texel_ids=ids, out=torch.zeros((K + 1, pos.shape[0], 3), device="cuda"))
    # an empty list never reaches the library
    out = torch.full((K, pos.shape[0], 3), SENTINEL, device="cuda")
    assert full.irt_multi(pos, nrm, shift, 64, tex, texel_ids=ids[:0], out=out) is out
    L = _lib.lib()
    Nt = pos.shape[0]
    need = int(L.texir_irt_multi_workspace_bytes(65, 64, K))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    dt = tex.cuda().permute(1, 2, 0, 3).contiguous()
    call = lambda n_ids, w, nbytes, sc=full, t=dt, k=K: L.texir_irt_multi(sc.h, _lib.ptr(pos), _lib.ptr(nrm), _lib.ptr(shift), _lib.ptr(ids), n_ids, Nt, 64, 0, _lib.ptr(t), k,
                                                                         _lib.ptr(out), _lib.ptr(w), nbytes, _lib.stream_ptr())
    with pytest.raises(_lib.TexirError, match="tex is null"):
        _lib.check(call(65, ws, need, t=None))
    with pytest.raises(_lib.TexirError, match="K must be in 1..8"):
        _lib.check(call(65, ws, need, t=None, k=9))               # K is reported before the null buffer
    with pytest.raises(_lib.TexirError, match="workspace"):
        _lib.check(call(65, ws, need - 1))
    with pytest.raises(_lib.TexirError, match="workspace"):
        _lib.check(call(65, None, need))
    _lib.check(call(0, None, 0))                                # a non-null empty list is a no-op, whatever the workspace
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    monkeypatch.setenv("TEXIR_BVH_WIDTH", "2")
    geo, _ = TC.golden_geo(MC.SCENE)
    binary = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    with pytest.raises(_lib.TexirError, match="4-wide tree"):
        _lib.check(call(65, ws, need, binary))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- 6. the bounce light of inserted emitters ----------------------------------------------------------------------------------------------------------------------

ATLAS = 32
_AT = {}


def atlas(tx):
    """a 32 x 32 texel atlas of the room in file orientation: (pos, nrm [Nt,3], shift [Nt,2], ids of the covered texels, prim [H,W])"""
    if not _AT:
        from texir_code_amd import gbuffer as GB
        full, _, _ = world(tx)
        pos, nrm, prim, _ = GB.raster_texel_gbuffer(full, ATLAS, ATLAS, offset=1e-2, want_ids=True)
        shift = torch.rand(ATLAS * ATLAS, 2, generator=torch.Generator().manual_seed(9)).cuda()
        ids = torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32)
        assert ids.numel() > 200
        _AT["v"] = (pos.reshape(-1, 3).contiguous(), nrm.reshape(-1, 3).contiguous(), shift, ids, prim)
    return _AT["v"]


def room_lights(tmp_path):
    geo, _ = TC.golden_geo(MC.SCENE)
    lo, hi = geo.verts.min(0).astype(np.float64), geo.verts.max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.3 * ext[0], 0, 0], [0, 0, 0.3 * ext[2]]
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                                         {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.1 * float(ext.min())}]}))
    return str(js), ctr


def test_bounce_is_irt_multi_of_the_bounce_textures(tx):
    from texir_code_amd import irtlight
    full, _, _ = world(tx)
    pos, nrm, shift, ids, _ = atlas(tx)
    g = torch.Generator().manual_seed(4)
    albedo = (0.8 * torch.rand(48, 40, 3, generator=g)).cuda()
    F = (3.0 * torch.rand(3, ATLAS, ATLAS, generator=g)).cuda()
    hw = full.tex_shape[:2]
    N = 64
    T1 = irtlight.bounce_textures(albedo, F, hw)
    g1 = full.irt_multi(pos, nrm, shift, N, T1, texel_ids=ids)
    G1 = irtlight.bounce(full, pos, nrm, shift, albedo, F, N, bounces=1, texel_ids=ids)
    assert torch.equal(G1, g1) and (g1 > 0).any() and (g1[:, ids.long()] > 0).any()
    T2 = irtlight.bounce_textures(albedo, g1.reshape(3, ATLAS, ATLAS, 3), hw)
    g2 = full.irt_multi(pos, nrm, shift, N, T2, texel_ids=ids)
    G2 = irtlight.bounce(full, pos, nrm, shift, albedo, F, N, bounces=2, texel_ids=ids, hw=(ATLAS, ATLAS))
    assert torch.equal(G2, g1 + g2) and (g2 > 0).any()
    # the ceiling: U = the estimator on the all-ones texture; no bounce gains energy
    U = full.irt_multi(pos, nrm, shift, N, torch.ones((1,) + tuple(hw) + (3,)), texel_ids=ids)[0].double()
    margin = 1.0 + (2 * N + 64) * 2.0 ** -24
    for name, G, T in (("G_1", g1, T1), ("G_2", g2, T2)):
        for k in range(3):
            top = float(T[k].max())
            assert (G[k].double() <= top * U * margin).all(), (name, k)
            print("%s[%d]: max %.4f under the ceiling max(T) max(U) = %.4f" % (name, k, float(G[k].max()), top * float(U.max())))
    assert float(albedo.max()) <= 0.8
    for k in range(3):
        assert float(g2[k].max()) <= 0.8 * float(U.max()) / np.pi * float(g1[k].max()) * margin, k


def test_orientation_pin_a_file_ramp_comes_back_as_its_own_row_and_column(tx):
    """a file-orientation image whose value is its own (row, column), through bounce_textures' orientation step and set_texture on a scratch scene: rays from
    the texel G-buffer's points along -n return that texel's (row, column).  Bilinear interpolation reproduces a linear ramp, and the hit lies on the
    texel centre up to the G-buffer's rounding, far below a texel"""
    from texir_code_amd import gbuffer as GB, irtlight
    geo, _ = TC.golden_geo(MC.SCENE)
    H = W = 2048                                                             # (the room's triangles are 0.19 / 64 of the atlas wide: 6 texels here)
    ramp = np.zeros((1, H, W, 3), np.float32)
    ramp[0, ..., 0], ramp[0, ..., 1] = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    one = np.full((1, 1, 3), irtlight.PI32, np.float32)                      # albedo / pi32 == 1 exactly
    T = irtlight.bounce_textures(one, ramp, (H, W))[0]
    assert np.array_equal(T.numpy(), ramp[0][::-1])
    scratch = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, np.zeros((H, W, 3), np.float32))
    scratch.set_texture(T)
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(scratch, H, W, offset=1e-2, want_ids=True)
    p = prim.cpu().numpy()
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner[1:-1, 1:-1] &= p[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] == p[1:-1, 1:-1]
    inner &= p >= 0
    rows, cols = np.nonzero(inner)
    assert len(rows) >= 100, len(rows)
    rows, cols = rows[::max(1, len(rows) // 4096)], cols[::max(1, len(cols) // 4096)]
    sel = torch.from_numpy(rows * W + cols).cuda()
    rad, t, pid, _ = scratch.trace_shade(pos.reshape(-1, 3)[sel], -nrm.reshape(-1, 3)[sel], return_hits=True)
    rad = rad.cpu().numpy()
    assert (pid.cpu().numpy() >= 0).all()
    err = np.maximum(np.abs(rad[:, 0] - rows), np.abs(rad[:, 1] - cols))
    print("orientation pin: %d texels, worst distance from the texel's own (row, column) %.4f texel" % (len(rows), err.max()))
    assert err.max() <= 0.05


def test_stage_writes_the_bounce_files_and_light_irt_adds_them(tmp_path, capsys):
    from texir_code_amd import datasets as D, io_formats as IO, irtlight, tools
    from texir_code_amd.trainer import exp_runner as ER

    def stage(tag, extra):
        root = str(tmp_path / tag)
        D.write_synthetic_dataset(root, T=2000, texel_res=64, tex_res=64, n_side=2)
        conf = str(tmp_path / (tag + ".conf"))
        D.write_conf(conf, root, cube_res=16, spp=(64, 16), model="irt")
        txt = open(conf).read()
        assert "batch_size = 1" in txt
        with open(conf, "w") as f:
            f.write(txt.replace("batch_size = 1", "batch_size = 1\n    " + "\n    ".join(extra), 1))
        d = os.path.join(root, "vrproc", "hdr_texture")
        before = set(os.listdir(d))
        ER.main(["--conf", conf, "--trainstage", "IrrT", "--gpu", "0"])
        return d, {f: open(os.path.join(d, f), "rb").read() for f in sorted(set(os.listdir(d)) - before)}

    probe = str(tmp_path / "probe")
    D.write_synthetic_dataset(probe, T=2000, texel_res=64, tex_res=64, n_side=2)
    verts = np.array([[float(v) for v in l.split()[1:4]] for l in open(os.path.join(probe, "vrproc", "hdr_texture", "out1.obj")) if l.startswith("v ")])
    lo, hi = verts.min(0), verts.max(0)
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.15 * ext[0], 0, 0], [0, 0, 0.15 * ext[2]]
    spec = {"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]},
                       {"kind": "sphere", "c": [ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], "r": 0.05 * float(ext.min())}]}
    js = str(tmp_path / "lights.json")
    with open(js, "w") as f:
        json.dump(spec, f)
    lights = ['irt_lights = "%s"' % js, "irt_light_samples = 16"]
    d0, plain = stage("plain", lights)
    d1, zero = stage("zero", lights + ["irt_light_bounces = 0", "irt_light_albedo = 0.5"])
    d2, one = stage("one", lights + ["irt_light_bounces = 1", "irt_light_albedo = 0.5", "irt_light_bounce_samples = 32"])
    assert "0_irr_texture_light1.hdr" in plain and not [f for f in plain if "bounce" in f]
    assert sorted(zero) == sorted(plain) and all(zero[f] == plain[f] for f in plain)
    assert sorted(set(one) - set(plain)) == ["0_irr_texture_light0_bounce.hdr", "0_irr_texture_light1_bounce.hdr"]
    assert all(one[f] == plain[f] for f in plain)
    rd = lambda name: IO.read_hdr(os.path.join(d2, name)).astype(np.float32)
    E = rd("0_irr_texture.hdr")
    F = np.stack([rd("0_irr_texture_light%d.hdr" % k)[..., 0] for k in (0, 1)])
    G = np.stack([rd("0_irr_texture_light%d_bounce.hdr" % k) for k in (0, 1)])
    for k in (0, 1):
        # albedo 0.5: what comes back is below the direct light's own maximum
        assert G[k].shape == E.shape and G[k].max() > 0 and G[k].max() < F[k].max()
        with capsys.disabled():
            print("stage: light %d: largest direct factor %.4f, largest bounce %.4f, bounce reaches %.1f %% of the atlas" % (k, F[k].max(), G[k].max(), 100.0 * (G[k].sum(-1) > 0).mean()))
    cols = [(20.0, 18.0, 15.0), (5.0, 5.0, 9.0)]
    argv = ["light-irt", d2, "--light", "0", "--colour", "20,18,15", "--light", "1", "--colour", "5,5,9"]
    assert tools.main(argv) == 0
    direct = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    os.remove(os.path.join(d2, "0_irr_texture_lit.hdr"))
    assert tools.main(argv + ["--bounce"]) == 0
    got = IO.read_hdr(os.path.join(d2, "0_irr_texture_lit.hdr")).astype(np.float64)
    want = irtlight.add_indirect(irtlight.add(E, F, cols), G, cols).astype(np.float64)
    # an RGBE pixel keeps 8 bits below its largest channel's power of two
    assert (np.abs(got - want) <= 2.0 ** -7 * want.max(-1)[..., None] + 1e-6 * want).all()
    assert (np.abs(direct - irtlight.add(E, F, cols)) <= 2.0 ** -7 * direct.max(-1)[..., None] + 1e-6 * direct).all() and got.sum() > direct.sum()
    capsys.readouterr()
    assert tools.main(["light-irt", d0, "--light", "0", "--colour", "1,1,1", "--bounce"]) == 1          # no bounce files there
    assert "train.irt_light_bounces" in capsys.readouterr().out
    # a required key that is missing names itself
    with pytest.raises(ValueError, match="train.irt_light_albedo"):
        stage("noalbedo", lights + ["irt_light_bounces = 1"])


def test_evaluation_model_with_light_bounces_adds_the_fetched_bounce_texture(tx, tmp_path):
    from texir_code_amd import cameras, gbuffer as GB, irtlight, texpost
    from texir_code_amd.tester import lit_model as LM, test_model as TM
    from texir_code_amd.texture import texture as tex_fetch
    full, _, _ = world(tx)
    js, ctr = room_lights(tmp_path)
    R = 64
    g = torch.Generator().manual_seed(12)
    par = lambda t: torch.nn.Parameter(t.cuda(), requires_grad=False)
    m = LM.MaterialModel.__new__(LM.MaterialModel)
    torch.nn.Module.__init__(m)
    m.scene, m.device = full, full.device
    m.sample_l, m.sample_type, m.relighting, m.cube_res = [16, 16], ["uniform", "importance"], False, 8
    m.materials_a = par(0.1 + 0.7 * torch.rand(R, R, 3, generator=g))
    m.materials_r = par(0.2 + 0.5 * torch.rand(R, R, 1, generator=g))
    m.irrt = par(torch.rand(R, R, 3, generator=g))
    m.texture_seg = par(torch.zeros(R, R, 1))
    m.max_mip_level = TM.get_mip_level(R)
    m._gb_cache = {}
    m.test_lights, m.light_samples = LM.load_test_lights(js, m.device), 32
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = ctr
    mvp, cam = cameras.cube_mvps(E)
    torch.manual_seed(5)
    absent = m(mvp, "v", cam, False)                                       # the attributes of the bounce absent: the model as it was
    state = torch.get_rng_state()
    m.light_bounces, m.light_bounce_samples, m.bounce_tex = 0, 64, None
    torch.manual_seed(5)
    zero = m(mvp, "v", cam, False)
    assert torch.equal(torch.get_rng_state(), state)
    assert sorted(zero) == sorted(absent) and all(torch.equal(zero[k], absent[k]) for k in zero), "0 bounces: the same outputs"
    # one bounce: built once, from a private generator
    m.light_bounces = 1
    torch.manual_seed(5)
    before = torch.get_rng_state()
    tex = m.build_bounce_texture()
    assert torch.equal(torch.get_rng_state(), before), "the texel shifts drew from the CPU generator"
    assert tuple(tex.shape) == (R, R, 3) and tex.is_cuda and (tex > 0).any() and torch.isfinite(tex).all()
    lit = m(mvp, "v", cam, False)
    assert torch.equal(torch.get_rng_state(), state) and getattr(m, "_bounce_irr", None) is None
    # the texture restated from the pieces
    records, colours = m.test_lights
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(full, R, R, normal="geometric", offset=1e-2, want_ids=True)
    covered = (prim >= 0).reshape(-1)
    ids = torch.nonzero(covered)[:, 0].to(torch.int32)
    shift = torch.rand(R * R, 2, generator=torch.Generator().manual_seed(LM.BOUNCE_SEED)).cuda()
    F = full.irt_lights(pos.reshape(-1, 3), nrm.reshape(-1, 3), shift, records, 32, texel_ids=ids).reshape(-1, R, R)
    assert (R, R) != tuple(full.tex_shape[:2])                              # (another grid than the radiance texture's: no gutter map)
    G = irtlight.bounce(full, pos.reshape(-1, 3), nrm.reshape(-1, 3), shift, m.materials_a.detach(), F, 64, bounces=1, texel_ids=ids, hw=(R, R))
    assert torch.equal(tex, irtlight.add_indirect(torch.zeros((R, R, 3), device="cuda"), G.reshape(-1, R, R, 3), colours))
    # the view: the 0-bounce rgb plus albedo / pi32 * the fetched texture, <= 2 ulp of the sum
    gb = m._gbuffer(mvp, "v")
    fetch = tex_fetch(tex, gb["uv"], gb["uv_da"], "linear-mipmap-linear", m.max_mip_level)
    pi = torch.tensor([irtlight.PI32], device="cuda")
    want = zero["rgb"].double() + (lit["albedo"] / pi * fetch).double()
    ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32))).cuda().double()
    assert ((lit["rgb"].double() - want).abs() <= 2 * ulp).all() and not torch.equal(lit["rgb"], zero["rgb"]) and (fetch > 0).any()
    for k in ("albedo", "normal", "position", "roughness", "empty_mask"):
        assert torch.equal(lit[k], zero[k])
