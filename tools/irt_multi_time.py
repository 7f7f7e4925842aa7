"""Time of the multi-texture IrT pass (texir_irt_multi, csrc/irtmulti.hip) against the route that gives the same answer without it.

    python tools/irt_multi_time.py [--workload c4] [--samples 2048,256] [--textures 2,8] [--repeats 5] [--slice 0] [--out profiles/irt_multi.json]

The scene, texel G-buffer and shifts of bench.py's workload (c4: 1M triangles, 4096^2 texels), the listed texels in Morton order (--slice n: the first n
of them; 0: all).  Per sample count and per K, in ONE process and alternately, repetition by repetition:
  * irt_multi on the K textures, handed over interleaved (Scene.irt_multi(interleaved=True));
  * the route without it: K x (set_texture(T_k) + irt_generate in its 64-texel form).
Timed besides, as figures of their own: the one permute().contiguous() that makes the interleaved copy, and the K set_texture re-tiles alone.  All times
are device-synchronised wall times with their spread (min, max); the two routes' outputs are asserted bit-identical.  The textures are the workload's own
radiance texture rolled by k * 97 rows and scaled by 1 + k / 8: K different textures of ordinary values.  The figures are recorded; no ratio is promised.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP = "irt_group_kernel<false, 4, 6>"


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
    ap.add_argument("--samples", default="2048,256", help="sample counts: the stage's and the evaluation model's bounce default")
    ap.add_argument("--textures", default="2,8")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice", type=int, default=0, help="time the first n listed texels only (0: the whole list)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_multi.json"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("irt_multi_time: at least 5 repetitions each")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_multi_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import _lib, dist_util
    from texir_code_amd.scene import Scene
    sc0, pos, nrm, valid, shift, res, _ = bench.make_workload(a.workload)
    hdr = np.ascontiguousarray(sc0["hdr"], np.float32)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], hdr, device=0)
    pos, nrm, shift = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    if a.slice > 0:
        ids = ids[:a.slice].contiguous()
    Nt, n = pos.shape[0], ids.numel()
    base = torch.from_numpy(hdr).cuda()
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "texels": [res, res], "texture": list(hdr.shape[:2]), "listed_texels": int(n),
           "sliced": bool(a.slice > 0), "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": []}
    L = _lib.lib()
    for K in (int(v) for v in a.textures.split(",")):
        planar = torch.stack([torch.roll(base, 97 * k, 0) * (1.0 + k / 8.0) for k in range(K)]).contiguous()
        permute = summary([wall_ms(lambda: planar.permute(1, 2, 0, 3).contiguous()) for _ in range(a.warmup + a.repeats)][a.warmup:])
        inter = planar.permute(1, 2, 0, 3).contiguous()
        retile = summary([wall_ms(lambda: [scene.set_texture(planar[k]) for k in range(K)]) for _ in range(a.warmup + a.repeats)][a.warmup:])
        for N in (int(v) for v in a.samples.split(",")):
            assert scene.irt_kernel_name(n, N) == GROUP, "the list is too short for the 64-texel form: %d texels" % n
            got = torch.zeros((K, Nt, 3), device="cuda")
            want = torch.zeros((K, Nt, 3), device="cuda")

            def multi():
                scene.irt_multi(pos, nrm, shift, N, inter, texel_ids=ids, out=got, interleaved=True)

            def route():
                for k in range(K):
                    scene.set_texture(planar[k])
                    scene.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, out=want[k])
            tm, tr = [], []
            for r in range(a.warmup + a.repeats):                 # alternately: both routes see the same drift of clocks and temperature
                m, s = wall_ms(multi), wall_ms(route)
                if r >= a.warmup:
                    tm.append(m)
                    tr.append(s)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "irt_multi and the set_texture route differ (K=%d, N=%d)" % (K, N)
            rec = {"K": K, "samples": N, "irt_multi": summary(tm), "set_texture_route": summary(tr), "permute_copy": permute, "set_texture_alone": retile,
                   "bit_identical": True, "workspace_bytes_per_texel": int(L.texir_irt_multi_workspace_bytes(1, N, K)),
                   "texture_bytes_interleaved": int(inter.numel()) * 4}
            rec["route_over_multi"] = round(rec["set_texture_route"]["median_ms"] / rec["irt_multi"]["median_ms"], 3)
            rec["route_spread_ms"] = round(rec["set_texture_route"]["max_ms"] - rec["set_texture_route"]["min_ms"], 3)
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
        scene.set_texture(base)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
