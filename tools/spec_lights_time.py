"""Time of the inserted lights' specular pass (texir_spec_lights, csrc/speclight.hip) beside the light pass on the same points.

    python tools/spec_lights_time.py [--workload c4] [--cube 512] [--samples 64] [--rounds 7] [--out profiles/spec_lights.json]

The scene of bench.py's workload (c4: 1M triangles), ONE view of 6 x cube^2 pixels cast from a camera of the grid (gbuffer.cast_gbuffer), the pixels in view
order, positions offset by 1e-2 normals as the material model offsets them, one ceiling quad and one sphere placed from the mesh's bounds as
tools/irt_lights_time.py places them, S samples per pixel, light and technique, roughness 0.1 / 0.5 on alternate pixels.  All in ONE process, the calls taken
in turn round by round (A B C D, A B C D, ...) so that clock and cache drift fall on all alike; HIP-event time per call; medians with min and max:
  * Scene.spec_lights query="closest" and query="any" (their results must agree bit for bit: recorded);
  * Scene.irt_lights query="closest" and query="any" on the same points: the pass that gives the diffuse half of the same relit view.
Recorded besides: stats (rays traced, visible ones) of both passes and the ratio spec / irt per query.  The figures are recorded, nothing is asserted here.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--t-max", type=float, default=0.999)
    ap.add_argument("--clamp-eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_lights.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spec_lights_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import cameras, gbuffer as GB, irtlight
    from texir_code_amd.scene import Scene
    sc0 = bench.make_workload(a.workload)[0]
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.ascontiguousarray(sc0["hdr"], np.float32), device=0)
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    ea, eb = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    records = irtlight.pack([irtlight.quad(np.array([ctr[0], hi[1] - 0.15 * ext[1], ctr[2]]) - ea / 2 - eb / 2, ea, eb),
                             irtlight.sphere([ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], 0.05 * float(ext.min()))])
    mvp, cam = cameras.cube_mvps(cameras.grid_cameras(4)[5])
    gb = GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True)
    P, S = 6 * a.cube * a.cube, a.samples
    nrm = gb["normal"].reshape(P, 3).contiguous()
    pos = (gb["position"].reshape(P, 3) + 1e-2 * nrm).contiguous()
    cam = cam.cuda().reshape(3).float().contiguous()
    rough = torch.where(torch.arange(P, device="cuda") % 2 == 0, 0.1, 0.5).float().contiguous()
    shift = torch.rand(P, 2, generator=torch.Generator().manual_seed(0)).cuda()
    rec_dev = torch.from_numpy(records).cuda()
    K = records.shape[0]
    R = {q: torch.zeros((K, P), device="cuda") for q in ("closest", "any")}
    F = {q: torch.zeros((K, P), device="cuda") for q in ("closest", "any")}
    calls = {}
    for q in ("closest", "any"):
        calls["spec_lights_" + q] = lambda q=q: scene.spec_lights(pos, nrm, rough, shift, cam, rec_dev, S, t_max=a.t_max, clamp_eps=a.clamp_eps, query=q, out=R[q])
        calls["irt_lights_" + q] = lambda q=q: scene.irt_lights(pos, nrm, shift, rec_dev, S, t_max=a.t_max, query=q, out=F[q])
    _, st_spec = scene.spec_lights(pos, nrm, rough, shift, cam, rec_dev, S, t_max=a.t_max, clamp_eps=a.clamp_eps, out=R["closest"], stats=True)
    _, st_irt = scene.irt_lights(pos, nrm, shift, rec_dev, S, t_max=a.t_max, out=F["closest"], stats=True)
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
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "view": [6, a.cube, a.cube], "pixels": P, "lights": records[:, :10].tolist(), "samples": S,
           "roughness": [0.1, 0.5], "t_max": a.t_max, "clamp_eps": a.clamp_eps, "warmup": a.warmup, "rounds": a.rounds, "order": list(calls),
           "device": torch.cuda.get_device_name(0)}
    for k, v in ts.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    out["spec_lights_stats"] = {"terms_traced": int(st_spec[0]), "visible": int(st_spec[1]), "terms_possible": P * K * S * 2}
    out["irt_lights_stats"] = {"rays_traced": int(st_irt[0]), "visible": int(st_irt[1]), "samples": P * K * S}
    out["any_equals_closest_bits"] = {"spec_lights": bool(torch.equal(R["closest"], R["any"])), "irt_lights": bool(torch.equal(F["closest"], F["any"]))}
    out["spec_over_irt"] = {q: round(out["spec_lights_" + q]["median_ms"] / out["irt_lights_" + q]["median_ms"], 3) for q in ("closest", "any")}
    out["lit_share"] = {"R": [round(float((R["closest"][k] > 0).float().mean()), 4) for k in range(K)], "F": [round(float((F["closest"][k] > 0).float().mean()), 4) for k in range(K)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
