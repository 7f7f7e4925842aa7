"""Time of the mesh-shadow pass (texir_irt_shadow_mesh, csrc/irtshadowmesh.hip) beside the estimator whose rays it selects from.

    python tools/irt_shadow_mesh_time.py [--workload c4] [--samples 2048,256] [--repeats 5] [--slice 0] [--merged] [--out profiles/irt_shadow_mesh.json]

The scene, texel G-buffer and shifts of bench.py's workload (c4: 1M triangles, 4096^2 texels), the listed texels in Morton order (--slice n: the first n
of them; 0: all), and two objects standing on the floor: a table (five boxes, every face a grid: 3 840 triangles) and a person-sized ellipsoid (4 512), with
the sets {0}, {1} and {0, 1}.  Per sample count, in ONE process and alternately, repetition by repetition: Scene.irt_shadow_mesh, and Scene.irt_generate on
the same texels, each timed with device events around the call; then the pass with prefilter=False.  Recorded: the medians with their spread (min, max: the
baseline's spread over its repeats tells a difference from noise), `stats` as shares of the estimator's rays, the ratio.  --merged: once, the functional
alternative -- the scene rebuilt with both objects merged in (host wall time of the build) and irt_generate on it.  No threshold is set: the claim is the
recorded ratio.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": len(ts)}


def grid_box(lo, hi, n):
    """a box whose faces are n x n grids: 12 n^2 triangles"""
    import numpy as np
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    vs, ts = [], []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, 1):
            base = len(vs)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = np.zeros(3)
                    p[ax] = (lo, hi)[side][ax]
                    p[u] = lo[u] + (hi[u] - lo[u]) * i / n
                    p[v] = lo[v] + (hi[v] - lo[v]) * j / n
                    vs.append(p)
            at = lambda i, j: base + i * (n + 1) + j
            for i in range(n):
                for j in range(n):
                    ts += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    return np.array(vs), np.array(ts, np.int32)


def table_mesh(n=8):
    import numpy as np
    parts = [grid_box([-0.7, 0.7, -0.45], [0.7, 0.76, 0.45], n)] + [grid_box([x - 0.05, 0.0, z - 0.05], [x + 0.05, 0.7, z + 0.05], n) for x in (-0.6, 0.6) for z in (-0.35, 0.35)]
    vs, ts, k = [], [], 0
    for v, t in parts:
        vs.append(v)
        ts.append(t + k)
        k += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts)


def person_mesh(n_lon=48, n_lat=48):
    """an ellipsoid 1.7 tall standing on y = 0: 2 n_lon (n_lat - 1) triangles"""
    import numpy as np
    v = [(0.0, 1.0, 0.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * (j + 0.5 * (i & 1)) / n_lon
            v.append((math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    t = [(0, ring(1, j + 1), ring(1, j)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            t += [(ring(i, j), ring(i, j + 1), ring(i + 1, j)), (ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j))]
    last = len(v) - 1
    t += [(last, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)) for j in range(n_lon)]
    return (np.array(v) * np.array([0.3, 0.85, 0.22]) + np.array([0.0, 0.85, 0.0])).astype(np.float32), np.array(t, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--samples", default="2048,256", help="sample counts: the stage's and the evaluation model's default")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice", type=int, default=0, help="time the first n listed texels only (0: the whole list)")
    ap.add_argument("--merged", action="store_true", help="also time, once, the rebuild of the scene with the objects merged in and irt_generate on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_shadow_mesh.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("irt_shadow_mesh_time: at least 5 repetitions each")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_shadow_mesh_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import dist_util
    from texir_code_amd.scene import Scene
    sc0, pos, nrm, valid, shift, res, _ = bench.make_workload(a.workload)
    hdr = np.ascontiguousarray(sc0["hdr"], np.float32)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], hdr, device=0)
    pos, nrm, shift = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    if a.slice > 0:
        ids = ids[:a.slice].contiguous()
    Nt, n = pos.shape[0], ids.numel()
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    # the objects are modelled in metres for a room 3 high; the pose scales them to this scene and sets them on its floor
    s = float(ext[1]) / 3.0
    c20, s20 = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    poses = np.array([[[s * c20, 0, s * s20, ctr[0] - 0.1 * ext[0]], [0, s, 0, lo[1]], [-s * s20, 0, s * c20, ctr[2]]],
                      [[s, 0, 0, ctr[0] + 0.15 * ext[0]], [0, s, 0, lo[1]], [0, 0, s, ctr[2] + 0.1 * ext[2]]]], np.float64)
    meshes = [table_mesh(), person_mesh()]
    occ = [Scene.occluder(v, t, device=0) for v, t in meshes]
    sets = torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda")
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "texels": [res, res], "listed_texels": int(n), "sliced": bool(a.slice > 0),
           "objects": [{"name": nm, "triangles": int(len(t)), "pose_object_to_world": p.tolist()} for nm, (v, t), p in zip(("table", "person"), meshes, poses)],
           "sets": [[0], [1], [0, 1]], "warmup": a.warmup, "repeats": a.repeats, "timer": "device events around each call", "device": torch.cuda.get_device_name(0), "cases": []}
    lost = torch.zeros((3, Nt, 3), device="cuda")
    irr = torch.zeros((Nt, 3), device="cuda")
    run = lambda N, **kw: scene.irt_shadow_mesh(pos, nrm, shift, N, occ, [0, 1], poses, sets=sets, texel_ids=ids, out=lost, **kw)
    for N in (int(v) for v in a.samples.split(",")):
        ts, tg = [], []
        for r in range(a.warmup + a.repeats):                     # alternately: both see the same drift of clocks and temperature
            t_s = event_ms(lambda: run(N))
            t_g = event_ms(lambda: scene.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, out=irr))
            if r >= a.warmup:
                ts.append(t_s)
                tg.append(t_g)
        _, st = run(N, stats=True)
        st = [int(v) for v in st.cpu().tolist()]
        keep = lost.clone()
        t_off = [event_ms(lambda: run(N, prefilter=False)) for _ in range(2)]
        assert torch.equal(keep, lost), "the prefilter changes a bit"
        sel = ids.long()
        assert bool((lost[2][sel] <= irr[sel] * (1 + 1e-3) + 1e-6).all()), "the shadow of both objects exceeds the irradiance it is a part of"
        rec = {"samples": N, "irt_shadow_mesh": summary(ts), "irt_generate": summary(tg), "irt_shadow_mesh_prefilter_off": summary(t_off),
               "kernel": scene.irt_kernel_name(n, N), "stats": st, "scene_rays_share_of_the_estimators_rays": round(st[0] / float(n * N), 6),
               "occluder_queries_share_of_the_estimators_rays": round(st[1] / float(n * N), 6), "blocked_share_of_the_estimators_rays": round(st[2] / float(n * N), 6),
               "largest_lost_over_irradiance": round(float((lost[2][sel].sum(-1) / irr[sel].sum(-1).clamp(min=1e-9)).max()), 4)}
        rec["generate_over_shadow_mesh"] = round(rec["irt_generate"]["median_ms"] / rec["irt_shadow_mesh"]["median_ms"], 3)
        rec["baseline_spread_over_median"] = round((rec["irt_generate"]["max_ms"] - rec["irt_generate"]["min_ms"]) / rec["irt_generate"]["median_ms"], 4)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.merged:
        # the functional alternative: one scene with the objects in it (they take the uv of the scene's first corner: their own radiance is not the question)
        N = int(a.samples.split(",")[0])
        vs, tr, uv = [np.asarray(sc0["verts"], np.float32)], [np.asarray(sc0["tris"], np.int32)], [np.asarray(sc0["tri_uvs"], np.float32).reshape(-1, 2)]
        k = len(vs[0])
        for (v, t), p in zip(meshes, poses):
            vs.append((v.astype(np.float64) @ p[:, :3].T + p[:, 3]).astype(np.float32))
            tr.append(t + k)
            uv.append(np.tile(uv[0][:1], (3 * len(t), 1)))
            k += len(v)
        t0 = time.perf_counter()
        merged = Scene(np.concatenate(vs), np.concatenate(tr), np.concatenate(uv), hdr, device=0)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        tm = [event_ms(lambda: merged.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, out=irr)) for _ in range(2)]
        out["merged_mesh_route"] = {"samples": N, "scene_build_wall_ms": round(build_ms, 1), "irt_generate": summary(tm), "runs_note": "first run includes any tuning"}
        print(json.dumps(out["merged_mesh_route"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
