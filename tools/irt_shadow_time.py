"""Time of the body-shadow pass (texir_irt_shadow, csrc/irtshadow.hip) beside the estimator whose rays it selects from.

    python tools/irt_shadow_time.py [--workload c4] [--samples 2048,256] [--repeats 5] [--slice 0] [--out profiles/irt_shadow.json]

The scene, texel G-buffer and shifts of bench.py's workload (c4: 1M triangles, 4096^2 texels), the listed texels in Morton order (--slice n: the first n
of them; 0: all), and the ceiling panel and the sphere of tools/irt_lights_time.py (profiles/irt_lights.json) as the two bodies, with the sets {0}, {1} and
{0, 1}.  Per sample count, in ONE process and alternately, repetition by repetition: Scene.irt_shadow, and Scene.irt_generate on the same texels.  All times
are device-synchronised wall times with their spread (min, max); `stats` (the samples whose ray met a body: the rays traced, and the blocked ones) is
recorded beside them, with the share of the estimator's rays that the pass traced.  No threshold is set: the claim is the recorded ratio.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--samples", default="2048,256", help="sample counts: the stage's and the evaluation model's default")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice", type=int, default=0, help="time the first n listed texels only (0: the whole list)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_shadow.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("irt_shadow_time: at least 5 repetitions each")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_shadow_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import dist_util, irtlight
    from texir_code_amd.scene import Scene
    sc0, pos, nrm, valid, shift, res, _ = bench.make_workload(a.workload)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.ascontiguousarray(sc0["hdr"], np.float32), device=0)
    pos, nrm, shift = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    if a.slice > 0:
        ids = ids[:a.slice].contiguous()
    Nt, n = pos.shape[0], ids.numel()
    lo, hi = sc0["verts"].min(0).astype(np.float64), sc0["verts"].max(0).astype(np.float64)
    ext, ctr = hi - lo, (hi + lo) / 2
    ea, eb = np.array([0.15 * ext[0], 0, 0]), np.array([0, 0, 0.15 * ext[2]])
    records = irtlight.pack([irtlight.quad(np.array([ctr[0], hi[1] - 0.15 * ext[1], ctr[2]]) - ea / 2 - eb / 2, ea, eb),
                             irtlight.sphere([ctr[0], lo[1] + 0.6 * ext[1], ctr[2]], 0.05 * float(ext.min()))])
    bodies = torch.from_numpy(records).cuda()
    sets = torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda")
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "texels": [res, res], "listed_texels": int(n), "sliced": bool(a.slice > 0),
           "bodies": [r[:10].tolist() for r in records], "sets": [[0], [1], [0, 1]], "warmup": a.warmup, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "cases": []}
    lost = torch.zeros((3, Nt, 3), device="cuda")
    irr = torch.zeros((Nt, 3), device="cuda")
    for N in (int(v) for v in a.samples.split(",")):
        ts, tg = [], []
        for r in range(a.warmup + a.repeats):                     # alternately: both see the same drift of clocks and temperature
            s = wall_ms(lambda: scene.irt_shadow(pos, nrm, shift, N, bodies, sets=sets, texel_ids=ids, out=lost))
            g = wall_ms(lambda: scene.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, out=irr))
            if r >= a.warmup:
                ts.append(s)
                tg.append(g)
        _, st = scene.irt_shadow(pos, nrm, shift, N, bodies, sets=sets, texel_ids=ids, out=lost, stats=True)
        st = [int(v) for v in st.cpu().tolist()]
        sel = ids.long()
        assert bool((lost[2][sel] <= irr[sel] * (1 + 1e-3) + 1e-6).all()), "the shadow of both bodies exceeds the irradiance it is a part of"
        rec = {"samples": N, "irt_shadow": summary(ts), "irt_generate": summary(tg), "kernel": scene.irt_kernel_name(n, N), "stats": st,
               "traced_share_of_the_estimators_rays": round(st[0] / float(n * N), 6), "blocked_share_of_the_traced": round(st[1] / max(st[0], 1), 4),
               "largest_lost_over_irradiance": round(float((lost[2][sel].sum(-1) / irr[sel].sum(-1).clamp(min=1e-9)).max()), 4)}
        rec["generate_over_shadow"] = round(rec["irt_generate"]["median_ms"] / rec["irt_shadow"]["median_ms"], 3)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
