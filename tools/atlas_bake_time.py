"""Time of the atlas bake (texir_atlas_bake, csrc/texbake.hip) and of the fill of what it leaves (texir_atlas_fill, csrc/texfill.hip) on one GPU.

    python tools/atlas_bake_time.py [--workload c4] [--views 16] [--pano 1024x2048] [--fill] [--fill-dist 0.5] [--fill-cos 0.5] [--out profiles/atlas_bake.json]

The scene of bench.py's workload (c4: 1M triangles, 4096^2 atlas), its texel G-buffer from the device rasteriser (gbuffer.raster_texel_gbuffer), --views
cameras on cameras.grid_cameras' grid, their panoramas from atlas.trace_panoramas, the covered texels in Morton order.  Recorded: the HIP-event median of
texir_atlas_bake (20 timed launches after 3 warm-up launches; launches only, every buffer made once), its `stats` counters and the rays per second they
imply, and, for scale, the texir_trace_shade ray rate on the panoramas' own rays measured in the same process.  No parent route computes the same thing:
the time is a recorded figure, not a threshold.  --fill adds texir_atlas_fill on the holes this bake leaves (sources: the covered texels with a view, holes:
those without, both in Morton order; the box of the scene's vertices grown by the G-buffer offset): the HIP-event median of the whole call (binning + search;
the same launch counts, or 1 + 5 when one call takes longer than two seconds), its `stats` counters and the cell edge the library chose.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 3, 20


def gpu_ms(fn, warmup=WARMUP, repeats=REPEATS):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--pano", default="1024x2048")
    ap.add_argument("--fill", action="store_true")
    ap.add_argument("--fill-dist", type=float, default=0.5)
    ap.add_argument("--fill-cos", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atlas_bake.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("atlas_bake_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import _lib, atlas, cameras, dist_util, gbuffer as GB, synth
    from texir_code_amd.scene import Scene
    T, res, tex_res, _, style = bench.WORKLOADS[a.workload]
    h, w = (int(v) for v in a.pano.lower().split("x"))
    n_side = int(round(math.sqrt(a.views)))
    if n_side * n_side != a.views:
        raise SystemExit("--views must be a square number (cameras.grid_cameras)")
    sc0 = synth.make_scene(T, seed=666, tex_res=tex_res, style=style)
    sc0["hdr"] = synth.rgbe_born(sc0["hdr"], 5.0)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], sc0["hdr"], device=0)
    E = np.stack(cameras.grid_cameras(n_side, room=synth.HOUSE) if style == "house" else cameras.grid_cameras(n_side), 0)
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(scene, res, res, want_ids=True)
    ids = dist_util.morton_order(torch.nonzero(prim.reshape(-1) >= 0)[:, 0].to(torch.int32), res).contiguous()
    Wm, cam = atlas.camera_matrices(E)
    Wm, cam = Wm.cuda().reshape(-1, 12).contiguous(), cam.cuda().contiguous()
    panos = atlas.trace_panoramas(scene, E, h, w).contiguous()
    pos, nrm = pos.reshape(-1, 3).contiguous(), nrm.reshape(-1, 3).contiguous()
    Nt = pos.shape[0]
    view = torch.empty(Nt, dtype=torch.int32, device="cuda")
    pix = torch.empty((Nt, 2), dtype=torch.int32, device="cuda")
    rgb = torch.empty((Nt, 3), dtype=torch.float32, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    L, p = _lib.lib(), _lib.ptr

    def bake(stats=None):
        _lib.check(L.texir_atlas_bake(scene.h, p(pos), p(nrm), p(ids), ids.numel(), Nt, p(Wm), p(cam), p(panos), None, a.views, h, w, 0.1, p(view), p(pix), p(rgb),
                                      p(stats), _lib.stream_ptr()))
    bake(st)
    torch.cuda.synchronize()
    counters = dict(zip(("pairs_facing", "pairs_traced", "pairs_visible", "texels_assigned"), (int(v) for v in st.cpu())))
    out = {"workload": a.workload, "triangles": T, "atlas": [res, res], "listed_texels": int(ids.numel()), "views": a.views, "panorama": [h, w],
           "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(0), "stats": counters}
    out["atlas_bake"] = gpu_ms(bake)
    out["atlas_bake"]["traced_rays_per_s"] = round(counters["pairs_traced"] / (out["atlas_bake"]["median_ms"] * 1e-3), 1)
    # for scale: texir_trace_shade on one panorama's rays (closest hit + the hit shader), same process
    d = atlas.pano_directions(atlas.camera_matrices(E)[0][0], h, w).to(torch.float32).reshape(-1, 3).cuda().contiguous()
    o = cam[0].expand_as(d).contiguous()
    rad = torch.empty_like(d)
    ts = gpu_ms(lambda: _lib.check(L.texir_trace_shade(scene.h, p(o), p(d), d.shape[0], 1e-4, p(rad), None, None, None, _lib.stream_ptr())))
    ts["rays"] = int(d.shape[0])
    ts["rays_per_s"] = round(d.shape[0] / (ts["median_ms"] * 1e-3), 1)
    out["trace_shade_panorama"] = ts
    if a.fill:
        import time
        seen = view[ids.long()] >= 0
        sources, holes = ids[seen].contiguous(), ids[~seen].contiguous()
        bounds = atlas.scene_bounds(sc0["verts"])
        src = torch.full((Nt,), -1, dtype=torch.int32, device="cuda")
        fst = torch.zeros(2, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(L.texir_atlas_fill_workspace_bytes(sources.numel(), holes.numel())), dtype=torch.uint8, device="cuda")

        def fill(stats=None):
            _lib.check(L.texir_atlas_fill(p(pos), p(nrm), Nt, p(sources), sources.numel(), p(holes), holes.numel(), p(bounds), a.fill_cos, a.fill_dist, 0.0, p(src), None,
                                          p(stats), p(ws), _lib.stream_ptr()))
        t0 = time.time()
        fill(fst)
        torch.cuda.synchronize()
        first_s = time.time() - t0
        wu, rp = (1, 5) if first_s > 2.0 else (WARMUP, REPEATS)
        fc = dict(zip(("holes_decided", "holes_filled"), (int(v) for v in fst.cpu())))
        out["atlas_fill"] = gpu_ms(fill, wu, rp)
        out["atlas_fill"].update({"warmup": wu, "repeats": rp, "sources": int(sources.numel()), "holes": int(holes.numel()), "fill_dist": a.fill_dist,
                                  "fill_cos": a.fill_cos, "cell": round(atlas.fill_cell(bounds, sources.numel()), 6), "bounds": [round(float(v), 4) for v in bounds],
                                  "workspace_bytes": int(ws.numel()), "stats": fc})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
