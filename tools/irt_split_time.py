"""Time of the irradiance split by source label (texir_irt_split, csrc/irtsplit.hip) against the route that gives the same answer without it.

    python tools/irt_split_time.py [--workload c4] [--repeats 3] [--out profiles/irt_split.json]

The scene, texel G-buffer, shifts and sample count of bench.py's workload (c4: 1M triangles, 4096^2 texels, 2048 spp), the listed texels in Morton order.
HIP-event medians, all in ONE process, of
  * the plain irt_generate;
  * irt_split at K = 2 (`lights`: irtsplit.labels_from_radiance) and at K = 8 (eight horizontal bands of the texture);
  * the route without the split for the same K textures: K x (set_texture(tex * [label == k]) + irt_generate), the masked textures made beforehand on the
    device, the full texture put back after the measurement.
Recorded besides: the ratios route / split, the spread (max - min) of the route's runs -- the split counts as faster only when it wins by more than that --
the workspace bytes and the number of list slices of each split.  The figures are recorded, nothing is asserted here.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gpu_ms(fn, warmup, repeats):
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
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-workspace-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_split.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_split_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import _lib, dist_util, irtsplit
    from texir_code_amd.scene import Scene
    sc0, pos, nrm, valid, shift, res, spp = bench.make_workload(a.workload)
    hdr = np.ascontiguousarray(sc0["hdr"], np.float32)
    scene = Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], hdr, device=0)
    pos, nrm, shift = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (pos.reshape(-1, 3), nrm.reshape(-1, 3), shift.reshape(-1, 2)))
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1) > 0))[:, 0].to(torch.int32).cuda(), res).contiguous()
    Nt, n = pos.shape[0], ids.numel()
    H, W = hdr.shape[:2]
    cap = int(a.max_workspace_gb * (1 << 30))
    label_sets = {"lights": (irtsplit.labels_from_radiance(hdr, 5.0), 2),
                  "bands8": (np.ascontiguousarray(np.broadcast_to((np.arange(H)[:, None] * 8 // H).astype(np.uint8), (H, W))), 8)}
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "texels": [res, res], "listed_texels": int(n), "spp": int(spp), "texture": [H, W],
           "texture_layout": scene.texture_layout(), "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    irr = torch.zeros((Nt, 3), device="cuda")
    plain = lambda: scene.irt_generate(pos, nrm, shift, spp, "uniform", texel_ids=ids, out=irr)
    plain()                                                     # (the scene's one-time scheduler measurement stays outside the timings)
    out["irt_generate"] = gpu_ms(plain, a.warmup, a.repeats)
    full_dev = torch.from_numpy(hdr).cuda()
    L = _lib.lib()
    for name, (lab, K) in label_sets.items():
        lab_dev = torch.from_numpy(lab).cuda()
        E = torch.zeros((K, Nt, 3), device="cuda")
        rec = {"K": K, "share_of_texels": [round(float((lab == k).mean()), 5) for k in range(K)]}
        per_texel = int(L.texir_irt_split_workspace_bytes(1, spp, K))
        step = n if per_texel * n <= cap else max(64, cap // per_texel // 64 * 64)
        rec["workspace_bytes"], rec["slices"] = int(per_texel * step), int((n + step - 1) // step)
        rec["irt_split"] = gpu_ms(lambda: scene.irt_split(pos, nrm, shift, spp, lab_dev, K, texel_ids=ids, out=E, max_workspace_bytes=cap), a.warmup, a.repeats)
        masked = [(full_dev * (lab_dev == k)[..., None]).contiguous() for k in range(K)]

        def route():
            for k in range(K):
                scene.set_texture(masked[k])
                scene.irt_generate(pos, nrm, shift, spp, "uniform", texel_ids=ids, out=irr)
        rec["masked_passes"] = gpu_ms(route, a.warmup, a.repeats)
        # the last masked pass against the split's last class: the same bits where the 64-texel form ran (lists of >= 32 768 texels)
        rec["last_class_equal_bits"] = bool(torch.equal(irr[ids.long()], E[K - 1][ids.long()]))
        scene.set_texture(full_dev)
        del masked
        r, s = rec["masked_passes"], rec["irt_split"]
        rec["route_over_split"] = round(r["median_ms"] / s["median_ms"], 3)
        rec["split_over_plain"] = round(s["median_ms"] / out["irt_generate"]["median_ms"], 3)
        rec["route_spread_ms"] = round(r["max_ms"] - r["min_ms"], 3)
        rec["faster_by_more_than_the_spread"] = bool(r["median_ms"] - s["median_ms"] > rec["route_spread_ms"])
        out[name] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
