"""Time of the specular shadow pass (texir_spec_shadow, csrc/specshadow.hip) beside spec_render on the same pixels.

    python tools/spec_shadow_time.py [--workload c4] [--cube 512] [--samples 64] [--rounds 7] [--out profiles/spec_shadow.json]

The scene of bench.py's workload (c4: 1M triangles), ONE view of 6 x cube^2 pixels cast from a camera of the grid (gbuffer.cast_gbuffer), the pixels in view
order, positions offset by 1e-2 normals as the material model offsets them, roughness 0.1 / 0.5 on alternate pixels (tools/spec_lights_time.py's view).  The
bodies are that tool's ceiling panel and sphere; the instances are the 3 840-triangle table and the 4 512-triangle person of tools/irt_shadow_mesh_time.py,
posed as that tool poses them; one set holding all four.  All in ONE process, the calls taken in turn round by round (A B C D E, A B C D E, ...) so that clock
and cache drift fall on all alike; HIP-event time per call; medians with min and max:
  * Scene.spec_shadow with the prefilter on and off (their results must agree bit for bit: ASSERTED), bodies only, instances only;
  * scene.spec_render on the same pixels: the pass whose specular term the shadow is a part of; its own spread over the rounds is recorded.
Recorded besides: stats (scene rays traced, occluder queries, blocked samples), the traced share of P * S, the share of pixels that lose anything.  No time is
asserted.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clamp-eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_shadow.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spec_shadow_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    import irt_shadow_mesh_time as MT
    from texir_code_amd import cameras, gbuffer as GB, irtlight
    from texir_code_amd.scene import Scene, spec_render
    sc0 = bench.make_workload(a.workload)[0]
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.ascontiguousarray(sc0["hdr"], np.float32), device=0)
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    ea, eb = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    records = irtlight.pack([irtlight.quad(np.array([ctr[0], hi[1] - 0.15 * ext[1], ctr[2]]) - ea / 2 - eb / 2, ea, eb),
                             irtlight.sphere([ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], 0.05 * float(ext.min()))])
    s = float(ext[1]) / 3.0
    c20, s20 = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    poses = np.array([[[s * c20, 0, s * s20, ctr[0] - 0.1 * ext[0]], [0, s, 0, lo[1]], [-s * s20, 0, s * c20, ctr[2]]],
                      [[s, 0, 0, ctr[0] + 0.15 * ext[0]], [0, s, 0, lo[1]], [0, 0, s, ctr[2] + 0.1 * ext[2]]]], np.float64)
    meshes = [MT.table_mesh(), MT.person_mesh()]
    occ = [Scene.occluder(v, t, device=0) for v, t in meshes]
    mvp, cam = cameras.cube_mvps(cameras.grid_cameras(4)[5])
    gb = GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True)
    P, S = 6 * a.cube * a.cube, a.samples
    nrm = gb["normal"].reshape(P, 3).contiguous()
    pos = (gb["position"].reshape(P, 3) + 1e-2 * nrm).contiguous()
    cam = cam.cuda().reshape(3).float().contiguous()
    rough = torch.where(torch.arange(P, device="cuda") % 2 == 0, 0.1, 0.5).float().contiguous()
    shift = torch.rand(P, 2, generator=torch.Generator().manual_seed(0)).cuda()
    rec_dev = torch.from_numpy(records).cuda()
    zero = torch.zeros((P, 3), device="cuda")
    forms = {"spec_shadow": dict(bodies=rec_dev, occluders=occ, instances=[0, 1], poses=poses), "spec_shadow_prefilter_off": dict(bodies=rec_dev, occluders=occ, instances=[0, 1],
                                                                                                                                 poses=poses, prefilter=False),
             "spec_shadow_bodies_only": dict(bodies=rec_dev), "spec_shadow_instances_only": dict(occluders=occ, instances=[0, 1], poses=poses)}
    outs = {k: torch.zeros((1, P, 3), device="cuda") for k in forms}
    calls = {k: (lambda k=k, kw=kw: scene.spec_shadow(pos, nrm, rough, shift, cam, S, clamp_eps=a.clamp_eps, out=outs[k], **kw)) for k, kw in forms.items()}
    calls["spec_render"] = lambda: spec_render(scene, nrm, zero, rough, pos, zero, cam, shift, S, clamp_eps=a.clamp_eps)
    stats = {k: [int(v) for v in scene.spec_shadow(pos, nrm, rough, shift, cam, S, clamp_eps=a.clamp_eps, out=outs[k], stats=True, **kw)[1].cpu()] for k, kw in forms.items()}
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    same = bool(torch.equal(outs["spec_shadow"], outs["spec_shadow_prefilter_off"]))
    assert same, "the prefilter changes a bit of out"
    assert stats["spec_shadow"][2] == stats["spec_shadow_prefilter_off"][2], "the prefilter changes the blocked count"
    term = calls["spec_render"]()
    lost = outs["spec_shadow"][0]
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "view": [6, a.cube, a.cube], "pixels": P, "samples": S, "roughness": [0.1, 0.5],
           "clamp_eps": a.clamp_eps, "bodies": records[:, :10].tolist(),
           "objects": [{"name": nm, "triangles": int(len(t)), "pose_object_to_world": p.tolist()} for nm, (v, t), p in zip(("table", "person"), meshes, poses)],
           "warmup": a.warmup, "rounds": a.rounds, "order": list(calls), "timer": "device events around each call", "device": torch.cuda.get_device_name(0)}
    for k, v in ts.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    out["spec_render_spread"] = round((max(ts["spec_render"]) - min(ts["spec_render"])) / statistics.median(ts["spec_render"]), 4)
    for k, st in stats.items():
        out[k + "_stats"] = {"scene_rays_traced": st[0], "occluder_queries": st[1], "blocked_samples": st[2], "traced_share_of_P_S": round(st[0] / float(P * S), 5)}
    out["prefilter_off_equals_on_bits"] = same
    out["shadow_over_render"] = {k: round(out[k]["median_ms"] / out["spec_render"]["median_ms"], 3) for k in forms}
    out["pixels_that_lose_light"] = round(float((lost > 0).any(1).float().mean()), 5)
    out["lost_within_the_term"] = bool(((lost >= 0) & (lost <= term)).all())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
