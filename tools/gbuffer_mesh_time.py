"""Time of the instanced cube G-buffer (texir_gbuffer_cast_mesh, csrc/gbuffermesh.hip) beside the plain one (texir_gbuffer_cast) on the same view.

    python tools/gbuffer_mesh_time.py [--workload c4] [--cube 512] [--rounds 7] [--out profiles/gbuffer_mesh.json]

The scene of bench.py's workload (c4: 1M triangles); ONE view of 6 x cube^2 pixels (tools/spec_lights_time.py's view); the table (3 840 triangles) and the
person (4 512) of tools/irt_shadow_mesh_time.py standing on the floor, posed as tools/irt_lights_mesh_time.py poses them.  All in ONE process, the calls taken
in turn round by round (A B C, A B C, ...) so that clock and cache drift fall on all alike; device-event time per call (the call allocates its outputs: both
forms alike); medians with min and max:
  * gbuffer.cast_gbuffer(occluders=...) with the prefilter on, and off (their results must agree bit for bit: asserted);
  * gbuffer.cast_gbuffer without objects -- the baseline: the code without this feature on the same view.
Recorded besides: the share of pixels that show an object, the new pass's time over the baseline's and the baseline's own spread.  The pixels that show the room
must hold the baseline's bits (asserted).  No target is set: a view's G-buffer is one ray per pixel and is cached per view; the claim is the recorded ratio.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbuffer_mesh.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("gbuffer_mesh_time: at least 5 rounds")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gbuffer_mesh_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    import irt_lights_mesh_time as LM
    import irt_shadow_mesh_time as SM
    from texir_code_amd import cameras, gbuffer as GB
    from texir_code_amd.scene import Scene, world_to_object
    sc0 = bench.make_workload(a.workload)[0]
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.ascontiguousarray(sc0["hdr"], np.float32), device=0)
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    s = float(ext[1]) / 3.0                                                        # the objects are modelled in metres for a room 3 high
    c20, s20 = math.cos(math.radians(20.0)), math.sin(math.radians(20.0))
    poses = np.array([[[s * c20, 0, s * s20, ctr[0] - 0.02 * ext[0]], [0, s, 0, lo[1]], [-s * s20, 0, s * c20, ctr[2]]],
                      [[s, 0, 0, ctr[0] + 0.15 * ext[0]], [0, s, 0, lo[1]], [0, 0, s, ctr[2] + 0.1 * ext[2]]]], np.float64)
    meshes = [SM.table_mesh(), SM.person_mesh()]
    occ = [Scene.occluder(v, t, device=0) for v, t in meshes]
    w2o = torch.from_numpy(world_to_object(poses)).cuda()
    mvp = cameras.cube_mvps(cameras.grid_cameras(4)[5])[0]
    res = {}
    calls = {"mesh_prefilter_on": lambda: res.__setitem__("on", GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True, occluders=occ, instances=[0, 1], poses=w2o)),
             "mesh_prefilter_off": lambda: res.__setitem__("off", GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True, occluders=occ, instances=[0, 1], poses=w2o,
                                                                                  prefilter=False)),
             "plain": lambda: res.__setitem__("plain", GB.cast_gbuffer(scene, mvp, a.cube, flip_v=True))}
    rec = LM.in_turn(calls, a.warmup, a.rounds)
    for k in res["on"]:
        assert torch.equal(res["on"][k], res["off"][k]), "the prefilter changes a bit of %s" % k
    room = res["on"]["inst_id"] < 0
    for k in res["plain"]:
        assert torch.equal(res["on"][k][room], res["plain"][k][room]), "a pixel that shows the room differs from the plain G-buffer in %s" % k
    P = 6 * a.cube * a.cube
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "view": [6, a.cube, a.cube], "pixels": P,
           "objects": [{"name": nm, "triangles": int(len(t)), "pose_object_to_world": p.tolist()} for nm, (v, t), p in zip(("table", "person"), meshes, poses)],
           "warmup": a.warmup, "rounds": a.rounds, "timer": "device events around each call, the calls in turn", "device": torch.cuda.get_device_name(0)}
    out.update(rec)
    out.update(pixels_that_show_an_object_share=round(float((~room).float().mean()), 6),
               pixels_per_instance=[int((res["on"]["inst_id"] == j).sum()) for j in range(2)],
               mesh_over_plain=round(rec["mesh_prefilter_on"]["median_ms"] / rec["plain"]["median_ms"], 3),
               prefilter_off_over_on=round(rec["mesh_prefilter_off"]["median_ms"] / rec["mesh_prefilter_on"]["median_ms"], 3),
               baseline_spread_over_median=round((rec["plain"]["max_ms"] - rec["plain"]["min_ms"]) / rec["plain"]["median_ms"], 4))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
