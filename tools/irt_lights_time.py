"""Time of the inserted-emitter pass (texir_irt_lights, csrc/irtlight.hip) and of the route that gives the same answer without it.

    python tools/irt_lights_time.py [--workload c4] [--samples 64] [--repeats 5] [--slice 1048576] [--out profiles/irt_lights.json]

The scene, texel G-buffer and shifts of bench.py's workload (c4: 1M triangles, 4096^2 texels), the listed texels in Morton order, one ceiling quad and one
sphere placed from the mesh's bounds, S samples per texel and light.  All in ONE process:
  * the HIP-event median of texir_irt_lights over the whole list, its stats (rays traced, visible ones) and the traced rays per second;
  * on a slice of the list (the first 1 M listed texels): the same call beside the route without it -- the sample points, directions and geometry terms
    built in torch ([n, S, 3] arrays), Scene.trace_shade(return_hits=True) on every ray, the visibility test and the sum over the samples in torch.
Recorded besides: the ratio route / kernel, the spread (max - min) of the route's runs -- the kernel counts as faster only when it wins by more than that --
the relative L2 between the two results and the bytes of ray arrays the route materialises.  The figures are recorded, nothing is asserted here.
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


def torch_route(scene, pos, nrm, shift, ids, records, S, t_max, chunk):
    """F [K, len(ids)] by the rule of include/texir_hip.h (texir_irt_lights) without the kernel: torch-built rays, trace_shade, a torch reduction"""
    import torch
    K = records.shape[0]
    out = torch.zeros((K, ids.numel()), device=pos.device)
    i = torch.arange(S, device=pos.device, dtype=torch.int64)
    h0 = (i.double() / S).float()
    rev = torch.zeros_like(i)
    v = i.clone()
    for _ in range(32):
        rev = (rev << 1) | (v & 1)
        v = v >> 1
    h1 = (rev.double() * 2.0 ** -32).float()

    def wrap(s):
        s = torch.where(s > 1, s - 1, s)
        s = torch.where(s < 0, s + 1, s)
        return s.clamp(1e-6, 1.0 - 1e-6)
    for first in range(0, ids.numel(), chunk):
        t = ids[first:first + chunk].long()
        x, n, sh = pos[t], nrm[t], shift[t]
        s0, s1 = wrap(h0[None, :] + sh[:, 0:1]), wrap(h1[None, :] + sh[:, 1:2])
        for k in range(K):
            rec = records[k]
            o, a, b = rec[1:4], rec[4:7], rec[7:10]
            if float(rec[0]) == 0.0:
                y = (o + s0[..., None] * a) + s1[..., None] * b
                m = torch.linalg.cross(a, b).expand_as(y)
                w = 1.0
            else:
                z = 1 - 2 * s0
                q = torch.sqrt(torch.clamp(1 - z * z, min=0))
                phi = 6.2831854820251465 * s1
                m = torch.stack([q * torch.cos(phi), q * torch.sin(phi), z], -1)
                y = o + a[0] * m
                w = 12.566370964050293 * float(a[0]) ** 2
            d = y - x[:, None, :]
            dd, nd, md = (d * d).sum(-1), (n[:, None, :] * d).sum(-1), -(m * d).sum(-1)
            g = (nd * md) / (dd * dd)
            g = torch.where((nd > 0) & (md > 0) & (dd > 0) & torch.isfinite(g), g, torch.zeros_like(g))
            _, th, pid, _ = scene.trace_shade(x[:, None, :].expand_as(d).reshape(-1, 3), d.reshape(-1, 3), t_min=0.0, return_hits=True)
            vis = ~((pid >= 0) & (th < t_max)).reshape(g.shape)
            out[k, first:first + len(t)] = (g * vis).sum(1) * (w / S)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slice", type=int, default=1 << 20)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="texels per torch pass of the route (its [n, S, 3] arrays are chunk * S * 12 bytes each)")
    ap.add_argument("--t-max", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irt_lights.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("irt_lights_time: needs a GPU (nothing is measured on a CPU)")
    import bench
    from texir_code_amd import dist_util, irtlight
    from texir_code_amd.scene import Scene
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
    out = {"workload": a.workload, "triangles": int(sc0["tris"].shape[0]), "texels": [res, res], "listed_texels": int(n), "lights": records[:, :10].tolist(), "samples": S,
           "t_max": a.t_max, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    F = torch.zeros((K, Nt), device="cuda")
    _, st = scene.irt_lights(pos, nrm, shift, rec_dev, S, texel_ids=ids, t_max=a.t_max, out=F, stats=True)
    whole = gpu_ms(lambda: scene.irt_lights(pos, nrm, shift, rec_dev, S, texel_ids=ids, t_max=a.t_max, out=F), a.warmup, a.repeats)
    traced, visible = (int(v) for v in st.cpu())
    out["irt_lights"] = dict(whole, rays_traced=traced, rays_visible=visible, samples=int(n) * K * S,
                             traced_rays_per_s=round(traced / (whole["median_ms"] * 1e-3), 1), lit_share=[round(float((F[k][ids.long()] > 0).float().mean()), 4) for k in range(K)])
    part = ids[:min(a.slice, n)].contiguous()
    rec = {"texels": int(part.numel()), "route_ray_array_bytes": int(part.numel()) * S * 12 * 2, "route_chunk": a.chunk}
    rec["irt_lights"] = gpu_ms(lambda: scene.irt_lights(pos, nrm, shift, rec_dev, S, texel_ids=part, t_max=a.t_max, out=F), a.warmup, a.repeats)
    rec["torch_route"] = gpu_ms(lambda: torch_route(scene, pos, nrm, shift, part, rec_dev, S, a.t_max, a.chunk), a.warmup, a.repeats)
    want = torch_route(scene, pos, nrm, shift, part, rec_dev, S, a.t_max, a.chunk)
    got = F[:, part.long()]
    rec["rel_l2"] = float(((got - want).double().norm() / want.double().norm().clamp_min(1e-30)).cpu())
    r, s = rec["torch_route"], rec["irt_lights"]
    rec["route_over_kernel"] = round(r["median_ms"] / s["median_ms"], 3)
    rec["route_spread_ms"] = round(r["max_ms"] - r["min_ms"], 3)
    rec["faster_by_more_than_the_spread"] = bool(r["median_ms"] - s["median_ms"] > rec["route_spread_ms"])
    out["slice"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
