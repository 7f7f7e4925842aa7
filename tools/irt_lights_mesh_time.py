"""Time of the inserted lights' passes with inserted mesh objects in the way (texir_irt_lights_mesh, csrc/irtlightmesh.hip; texir_spec_lights_mesh,
csrc/speclightmesh.hip) beside the object-free passes on the same points.

    python tools/irt_lights_mesh_time.py [--workload c4] [--samples 64] [--cube 512] [--rounds 7] [--out profiles/irt_lights_mesh.json]

The scene, texel G-buffer and shifts of bench.py's workload (c4: 1M triangles, 4096^2 texels), the listed texels in Morton order; the ceiling panel and the
sphere of tools/irt_lights_time.py; the table (3 840 triangles) and the person (4 512) of tools/irt_shadow_mesh_time.py standing on the floor.  All in ONE
process, the calls taken in turn round by round (A B C D, A B C D, ...) so that clock and cache drift fall on all alike; device-event time per call; medians
with min and max:
  * Scene.irt_lights(occluders=...) with the prefilter on, and off (their results must agree bit for bit: asserted);
  * Scene.irt_lights(query="any") without objects -- the baseline: the code without this feature on the same texels;
  * the merged-mesh route: the scene rebuilt with the posed objects in it (host wall time of the build, once), then irt_lights(query="any") on it.
The same four for Scene.spec_lights on ONE view of 6 x cube^2 pixels (tools/spec_lights_time.py's view).  Recorded besides: stats of every pass, the new
pass's time over the baseline's, the baseline's spread, and the share of traced segments that queried an object.  The kernels' stats stay (traced, visible),
so that share comes from a float32 restatement of the box test in torch on every --share-stride-th listed point (no padding: an estimate, the kernel's
padded test passes a few more).  No threshold is set: the claim is the recorded ratio.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


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


def in_turn(calls, warmup, rounds):
    ts = {k: [] for k in calls}
    for r in range(warmup + rounds):
        for k, fn in calls.items():
            t = event_ms(fn)
            if r >= warmup:
                ts[k].append(t)
    return {k: summary(v) for k, v in ts.items()}


def queried_share(pos, nrm, shift, records, S, w2o, boxes, stride):
    """share of the segments with g > 0 of every stride-th point whose object-space LINE meets some instance's box ahead of the point (light samples of the
    rule, float32 torch, unpadded slabs)"""
    import torch
    x, n, sh = pos[::stride], nrm[::stride], shift[::stride]
    i = torch.arange(S, device=x.device)
    rev = torch.zeros(S, device=x.device, dtype=torch.float64)
    for b in range(32):
        rev += ((i >> b) & 1).double() * 2.0 ** (-(b + 1))

    def wrap(s):
        s = torch.where(s > 1, s - 1, s)
        s = torch.where(s < 0, s + 1, s)
        return s.clamp(1e-6, 1 - 1e-6)
    s0 = wrap((i.double() / S).float()[None] + sh[:, :1])
    s1 = wrap(rev.float()[None] + sh[:, 1:])
    live_n, ask_n = 0, 0
    for rec in records:
        o, a, b = rec[1:4], rec[4:7], rec[7:10]
        if float(rec[0]) == 0.0:
            y = o + s0[..., None] * a + s1[..., None] * b
            m = torch.linalg.cross(a, b).expand_as(y)
        else:
            z = 1 - 2 * s0
            q = torch.sqrt((1 - z * z).clamp(min=0))
            phi = 2 * math.pi * s1
            m = torch.stack([q * torch.cos(phi), q * torch.sin(phi), z], -1)
            y = o + a[0] * m
        d = y - x[:, None]
        live = ((n[:, None] * d).sum(-1) > 0) & (-(m * d).sum(-1) > 0)
        ask = torch.zeros_like(live)
        for W, (blo, bhi) in zip(w2o, boxes):
            A, t = W[:, :3], W[:, 3]
            oo, dd = (x @ A.T + t)[:, None], d @ A.T
            inv = 1.0 / dd
            t0, t1 = (blo - oo) * inv, (bhi - oo) * inv
            tn, tf = torch.minimum(t0, t1).amax(-1), torch.maximum(t0, t1).amin(-1)
            ask |= (tn <= tf) & (tf > 0)
        live_n += int(live.sum())
        ask_n += int((live & ask).sum())
    return ask_n / max(live_n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--slice", type=int, default=0, help="time the first n listed texels only (0: the whole list)")
    ap.add_argument("--share-stride", type=int, default=64)
    ap.add_argument("--t-max", type=float, default=0.999)
    ap.add_argument("--clamp-eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_lights_mesh.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("irt_lights_mesh_time: at least 5 rounds")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_lights_mesh_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    import irt_shadow_mesh_time as SM
    from texir_code_amd import cameras, dist_util, gbuffer as GB, irtlight
    from texir_code_amd.scene import Scene, world_to_object
    sc0, pos, nrm, valid, shift, res, _ = bench.make_workload(a.workload)
    hdr = np.ascontiguousarray(sc0["hdr"], np.float32)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], hdr, device=0)
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    ea, eb = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    records = irtlight.pack([irtlight.quad(np.array([ctr[0], hi[1] - 0.15 * ext[1], ctr[2]]) - ea / 2 - eb / 2, ea, eb),
                             irtlight.sphere([ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], 0.05 * float(ext.min()))])
    rec_dev = torch.from_numpy(records).cuda()
    K, S = records.shape[0], a.samples
    # the objects are modelled in metres for a room 3 high; the pose scales them to this scene and sets them on its floor: the table under the lights
    s = float(ext[1]) / 3.0
    c20, s20 = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    poses = np.array([[[s * c20, 0, s * s20, ctr[0] - 0.02 * ext[0]], [0, s, 0, lo[1]], [-s * s20, 0, s * c20, ctr[2]]],
                      [[s, 0, 0, ctr[0] + 0.15 * ext[0]], [0, s, 0, lo[1]], [0, 0, s, ctr[2] + 0.1 * ext[2]]]], np.float64)
    meshes = [SM.table_mesh(), SM.person_mesh()]
    occ = [Scene.occluder(v, t, device=0) for v, t in meshes]
    w2o = torch.from_numpy(world_to_object(poses)).cuda()
    obj = dict(occluders=occ, instances=[0, 1], poses=w2o)
    boxes = [(torch.from_numpy(v.min(0)).cuda(), torch.from_numpy(v.max(0)).cuda()) for v, _ in meshes]
    # the merged-mesh route's scene (the objects take the uv of the scene's first corner: their own radiance is not the question)
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
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "lights": records[:, :10].tolist(), "samples": S, "t_max": a.t_max,
           "objects": [{"name": nm, "triangles": int(len(t)), "pose_object_to_world": p.tolist()} for nm, (v, t), p in zip(("table", "person"), meshes, poses)],
           "warmup": a.warmup, "rounds": a.rounds, "timer": "device events around each call, the calls in turn", "device": torch.cuda.get_device_name(0),
           "merged_scene_build_wall_ms": round(build_ms, 1)}

    def measure(call, plain, on_merged):
        res_ = {q: None for q in ("on", "off")}
        calls = {"mesh_prefilter_on": lambda: res_.__setitem__("on", call(prefilter=True)), "mesh_prefilter_off": lambda: res_.__setitem__("off", call(prefilter=False)),
                 "plain_any": plain, "merged_mesh_any": on_merged}
        rec = in_turn(calls, a.warmup, a.rounds)
        assert torch.equal(res_["on"], res_["off"]), "the prefilter changes a bit"
        return rec

    # ---- the atlas: irt_lights
    posd, nrmd, shiftd = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    if a.slice > 0:
        ids = ids[:a.slice].contiguous()
    Nt, n = posd.shape[0], ids.numel()
    F = {q: torch.zeros((K, Nt), device="cuda") for q in ("on", "off", "plain", "merged")}
    lights = lambda sc_, key, **kw: sc_.irt_lights(posd, nrmd, shiftd, rec_dev, S, texel_ids=ids, t_max=a.t_max, out=F[key], **kw)
    rec = measure(lambda prefilter: lights(scene, "on" if prefilter else "off", prefilter=prefilter, **obj), lambda: lights(scene, "plain", query="any"),
                  lambda: lights(merged, "merged", query="any"))
    st_mesh = [int(v) for v in lights(scene, "on", stats=True, **obj)[1].cpu()]
    st_plain = [int(v) for v in lights(scene, "plain", query="any", stats=True)[1].cpu()]
    st_merged = [int(v) for v in lights(merged, "merged", query="any", stats=True)[1].cpu()]
    sel = ids.long()
    assert bool((F["on"][:, sel] <= F["plain"][:, sel]).all()), "an object adds light"
    rec.update(texels=[res, res], listed_texels=int(n), sliced=bool(a.slice > 0), stats_mesh=st_mesh, stats_plain=st_plain, stats_merged_mesh=st_merged,
               mesh_over_plain=round(rec["mesh_prefilter_on"]["median_ms"] / rec["plain_any"]["median_ms"], 3),
               prefilter_off_over_on=round(rec["mesh_prefilter_off"]["median_ms"] / rec["mesh_prefilter_on"]["median_ms"], 3),
               merged_over_mesh=round(rec["merged_mesh_any"]["median_ms"] / rec["mesh_prefilter_on"]["median_ms"], 3),
               baseline_spread_over_median=round((rec["plain_any"]["max_ms"] - rec["plain_any"]["min_ms"]) / rec["plain_any"]["median_ms"], 4),
               segments_blocked_by_objects_share=round((st_plain[1] - st_mesh[1]) / max(st_plain[0], 1), 6),
               segments_that_queried_an_object_share=round(queried_share(posd[sel], nrmd[sel], shiftd[sel], rec_dev, S, w2o.reshape(-1, 3, 4), boxes, a.share_stride), 6),
               largest_value_differs_from_merged=round(float((F["on"][:, sel] - F["merged"][:, sel]).abs().max()), 6))
    out["irt_lights"] = rec
    print(json.dumps({"irt_lights": rec}), flush=True)

    # ---- one view: spec_lights
    mvp, cam = cameras.cube_mvps(cameras.grid_cameras(4)[5])
    gb = GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True)
    P = 6 * a.cube * a.cube
    vn = gb["normal"].reshape(P, 3).contiguous()
    vp = (gb["position"].reshape(P, 3) + 1e-2 * vn).contiguous()
    cam = cam.cuda().reshape(3).float().contiguous()
    rough = torch.where(torch.arange(P, device="cuda") % 2 == 0, 0.1, 0.5).float().contiguous()
    vshift = torch.rand(P, 2, generator=torch.Generator().manual_seed(0)).cuda()
    R = {q: torch.zeros((K, P), device="cuda") for q in ("on", "off", "plain", "merged")}
    spec = lambda sc_, key, **kw: sc_.spec_lights(vp, vn, rough, vshift, cam, rec_dev, S, t_max=a.t_max, clamp_eps=a.clamp_eps, out=R[key], **kw)
    rec = measure(lambda prefilter: spec(scene, "on" if prefilter else "off", prefilter=prefilter, **obj), lambda: spec(scene, "plain", query="any"),
                  lambda: spec(merged, "merged", query="any"))
    st_mesh = [int(v) for v in spec(scene, "on", stats=True, **obj)[1].cpu()]
    st_plain = [int(v) for v in spec(scene, "plain", query="any", stats=True)[1].cpu()]
    assert bool((R["on"] <= R["plain"]).all()), "an object adds light"
    rec.update(view=[6, a.cube, a.cube], pixels=P, stats_mesh=st_mesh, stats_plain=st_plain,
               mesh_over_plain=round(rec["mesh_prefilter_on"]["median_ms"] / rec["plain_any"]["median_ms"], 3),
               prefilter_off_over_on=round(rec["mesh_prefilter_off"]["median_ms"] / rec["mesh_prefilter_on"]["median_ms"], 3),
               merged_over_mesh=round(rec["merged_mesh_any"]["median_ms"] / rec["mesh_prefilter_on"]["median_ms"], 3),
               baseline_spread_over_median=round((rec["plain_any"]["max_ms"] - rec["plain_any"]["min_ms"]) / rec["plain_any"]["median_ms"], 4),
               segments_blocked_by_objects_share=round((st_plain[1] - st_mesh[1]) / max(st_plain[0], 1), 6))
    out["spec_lights"] = rec
    print(json.dumps({"spec_lights": rec}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
