"""Time of the any-hit forms against the closest-hit calls they shadow, measured alternately in ONE process.

    python tools/occlusion_time.py [--workload c4] [--samples 64] [--views 16] [--pano 1024x2048] [--repeats 7] [--out profiles/occlusion.json]

  (a) lights   tools/irt_lights_time.py's configuration (the workload's whole Morton-ordered list, one ceiling quad and one sphere, S samples):
               texir_irt_lights and texir_irt_lights_any in turn;
  (b) bake     tools/atlas_bake_time.py's configuration (the rasterised G-buffer, --views cameras, their traced panoramas):
               texir_atlas_bake and texir_atlas_bake_any in turn;
  (c) query    texir_trace_occluded against texir_trace_shade with all hit outputs, in rays per second, on the quad light's own rays (g > 0) of the first
               --slice listed texels with t_far = --t-max, and on the panorama rays of view 0 with t_far = inf.
HIP-event medians of --repeats runs after --warmup, min and max beside them.  THE BAR of (a) and (b): the any-hit call's median is below the closest-hit
call's by more than the closest-hit call's own max - min (`faster_by_more_than_the_spread`).  Whether the two forms returned the same bits is recorded
too (`same_bits`).  The figures are recorded, nothing is asserted here.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def alternate_ms(fns, warmup, repeats):
    """the calls of `fns` (name -> callable) timed in turn, round after round -> name -> {median_ms, min_ms, max_ms}"""
    import torch
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ts.items()}


def verdict(rec, base, new):
    b, n = rec[base], rec[new]
    rec["closest_over_any"] = round(b["median_ms"] / n["median_ms"], 4)
    rec["closest_spread_ms"] = round(b["max_ms"] - b["min_ms"], 4)
    rec["faster_by_more_than_the_spread"] = bool(b["median_ms"] - n["median_ms"] > rec["closest_spread_ms"])


def query_pair(scene, o, d, t_far, warmup, repeats):
    """texir_trace_occluded against texir_trace_shade(return_hits) on the rays (o, d)"""
    import torch
    from texir_code_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    R = o.shape[0]
    rad, t, uv = torch.empty((R, 3), device="cuda"), torch.empty(R, device="cuda"), torch.empty((R, 2), device="cuda")
    pid = torch.empty(R, dtype=torch.int32, device="cuda")
    occ = torch.empty(R, dtype=torch.uint8, device="cuda")
    fns = {"trace_shade_hits": lambda: _lib.check(L.texir_trace_shade(scene.h, p(o), p(d), R, 0.0, p(rad), p(t), p(pid), p(uv), _lib.stream_ptr())),
           "trace_occluded": lambda: _lib.check(L.texir_trace_occluded(scene.h, p(o), p(d), R, 0.0, t_far, p(occ), None, _lib.stream_ptr()))}
    rec = alternate_ms(fns, warmup, repeats)
    for k in fns:
        rec[k]["rays_per_s"] = round(R / (rec[k]["median_ms"] * 1e-3), 1)
    want = (pid >= 0) & (t < t_far)
    rec.update(rays=int(R), t_far=t_far if math.isfinite(t_far) else "inf", occluded_share=round(float(occ.float().mean()), 4),
               same_bits=bool(torch.equal(occ.bool(), want)))
    verdict(rec, "trace_shade_hits", "trace_occluded")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--pano", default="1024x2048")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slice", type=int, default=1 << 20)
    ap.add_argument("--t-max", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("occlusion_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import _lib, atlas, cameras, dist_util, gbuffer as GB, irtlight, synth
    from texir_code_amd.scene import Scene
    L, p = _lib.lib(), _lib.ptr
    out = {"workload": a.workload, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}

    # ---- (a) the light pass: tools/irt_lights_time.py's configuration ----
    sc0, pos, nrm, valid, shift, res, _ = bench.make_workload(a.workload)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.ascontiguousarray(sc0["hdr"], np.float32), device=0)
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    ea, eb = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    records = irtlight.pack([irtlight.quad(np.array([ctr[0], hi[1] - 0.15 * ext[1], ctr[2]]) - ea / 2 - eb / 2, ea, eb),
                             irtlight.sphere([ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], 0.05 * float(ext.min()))])
    pos, nrm, shift = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    rec_dev = torch.from_numpy(records).cuda()
    Nt, n, K, S = pos.shape[0], ids.numel(), records.shape[0], a.samples
    F = {q: torch.zeros((K, Nt), device="cuda") for q in ("closest", "any")}
    st = {q: torch.zeros(2, dtype=torch.int64, device="cuda") for q in F}

    def lights(q, stats=None):
        fn = L.texir_irt_lights_any if q == "any" else L.texir_irt_lights
        _lib.check(fn(scene.h, p(pos), p(nrm), p(shift), p(ids), n, Nt, p(rec_dev), K, S, a.t_max, p(F[q]), p(stats), _lib.stream_ptr()))
    for q in F:
        lights(q, st[q])
    torch.cuda.synchronize()
    rec = alternate_ms({"irt_lights": lambda: lights("closest"), "irt_lights_any": lambda: lights("any")}, a.warmup, a.repeats)
    traced, visible = (int(v) for v in st["closest"].cpu())
    rec.update(triangles=int(sc0["tris"].shape[0]), texels=[res, res], listed_texels=int(n), samples=S, t_max=a.t_max, rays_traced=traced, rays_visible=visible,
               occluded_share=round(1.0 - visible / max(traced, 1), 4), same_bits=bool(torch.equal(F["closest"], F["any"]) and torch.equal(st["closest"], st["any"])))
    verdict(rec, "irt_lights", "irt_lights_any")
    out["lights"] = rec

    # ---- (c1) the stand-alone query on the quad light's own rays of a slice ----
    part = ids[:min(a.slice, n)].long()
    x, nn, sh = pos[part], nrm[part], shift[part]
    i = torch.arange(S, device="cuda", dtype=torch.int64)
    h0 = (i.double() / S).float()
    rev, v = torch.zeros_like(i), i.clone()
    for _ in range(32):
        rev = (rev << 1) | (v & 1)
        v = v >> 1
    h1 = (rev.double() * 2.0 ** -32).float()

    def wrap(s):
        s = torch.where(s > 1, s - 1, s)
        s = torch.where(s < 0, s + 1, s)
        return s.clamp(1e-6, 1.0 - 1e-6)
    s0, s1 = wrap(h0[None, :] + sh[:, 0:1]), wrap(h1[None, :] + sh[:, 1:2])
    r0 = rec_dev[0]
    y = (r0[1:4] + s0[..., None] * r0[4:7]) + s1[..., None] * r0[7:10]
    m = torch.linalg.cross(r0[4:7], r0[7:10])
    d = y - x[:, None, :]
    need = ((nn[:, None, :] * d).sum(-1) > 0) & (-(m * d).sum(-1) > 0) & ((d * d).sum(-1) > 0)
    o = x[:, None, :].expand_as(d)[need].contiguous()
    d = d[need].contiguous()
    del y, s0, s1, need
    out["query_light_rays"] = query_pair(scene, o, d, a.t_max, a.warmup, a.repeats)
    out["query_light_rays"]["texels"] = int(part.numel())
    del o, d, scene, F
    torch.cuda.empty_cache()

    # ---- (b) the bake: tools/atlas_bake_time.py's configuration ----
    T, res, tex_res, _, style = bench.WORKLOADS[a.workload]
    h, w = (int(v) for v in a.pano.lower().split("x"))
    n_side = int(round(math.sqrt(a.views)))
    if n_side * n_side != a.views:
        raise SystemExit("--views must be a square number (cameras.grid_cameras)")
    sb = synth.make_scene(T, seed=666, tex_res=tex_res, style=style)
    sb["hdr"] = synth.rgbe_born(sb["hdr"], 5.0)
    scene = Scene(sb["verts"], sb["tris"], sb["tri_uvs"], sb["hdr"], device=0)
    E = np.stack(cameras.grid_cameras(n_side, room=synth.HOUSE) if style == "house" else cameras.grid_cameras(n_side), 0)
    bpos, bnrm, prim, _ = GB.raster_texel_gbuffer(scene, res, res, want_ids=True)
    bids = dist_util.morton_order(torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32), res).contiguous()
    Wm, cam = atlas.camera_matrices(E)
    Wm, cam = Wm.cuda().reshape(-1, 12).contiguous(), cam.cuda().contiguous()
    panos = atlas.trace_panoramas(scene, E, h, w).contiguous()
    bpos, bnrm = bpos.reshape(-1, 3).contiguous(), bnrm.reshape(-1, 3).contiguous()
    Nb = bpos.shape[0]
    res_b = {q: (torch.full((Nb,), -2, dtype=torch.int32, device="cuda"), torch.zeros((Nb, 2), dtype=torch.int32, device="cuda"),
                 torch.zeros((Nb, 3), dtype=torch.float32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")) for q in ("closest", "any")}

    def bake(q, stats=False):
        view, pix, rgb, bst = res_b[q]
        fn = L.texir_atlas_bake_any if q == "any" else L.texir_atlas_bake
        _lib.check(fn(scene.h, p(bpos), p(bnrm), p(bids), bids.numel(), Nb, p(Wm), p(cam), p(panos), None, a.views, h, w, 0.1, p(view), p(pix), p(rgb),
                      p(bst) if stats else None, _lib.stream_ptr()))
    for q in res_b:
        bake(q, True)
    torch.cuda.synchronize()
    rec = alternate_ms({"atlas_bake": lambda: bake("closest"), "atlas_bake_any": lambda: bake("any")}, a.warmup, a.repeats)
    counters = dict(zip(("pairs_facing", "pairs_traced", "pairs_visible", "texels_assigned"), (int(v) for v in res_b["closest"][3].cpu())))
    rec.update(triangles=T, atlas=[res, res], listed_texels=int(bids.numel()), views=a.views, panorama=[h, w], stats=counters,
               occluded_share=round(1.0 - counters["pairs_visible"] / max(counters["pairs_traced"], 1), 4),
               same_bits=bool(all(torch.equal(x, y) for x, y in zip(res_b["closest"], res_b["any"]))))
    verdict(rec, "atlas_bake", "atlas_bake_any")
    out["bake"] = rec

    # ---- (c2) the stand-alone query on the panorama rays of view 0, the whole ray ----
    d = atlas.pano_directions(atlas.camera_matrices(E)[0][0], h, w).to(torch.float32).reshape(-1, 3).cuda().contiguous()
    o = cam[0].expand_as(d).contiguous()
    out["query_panorama_rays"] = query_pair(scene, o, d, float("inf"), a.warmup, a.repeats)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
