"""Times of the uv-space texel rasteriser (csrc/texraster.hip, gbuffer.raster_texel_gbuffer) on one GPU, in one process.

    python tools/texel_raster_time.py [--no-stage] [--out profiles/texel_raster.json]

Kernels: texir_texel_gbuffer (all four launches) at 4096^2 on the c4 scene (1 M-triangle room) and on the house scene (1 M triangles: millimetre clutter next to
an untessellated shell), median of 20 HIP-event times after 3 warm-up rounds, workspace and outputs allocated once as a recorded graph would hold them.
`min_bytes` = what the call must write at least (pos + nrm [+ prim_id + bary]); `share_of_copy_rate` = that over the time over the device-to-device copy
rate measured in the same process (a 1 GiB torch copy counts read + write).  Stage: the `texel_gbuffer` phase of `--trainstage IrrT` at c4 for the three
routes -- raster, file, pano -- from ONE call of tools/stage_time.py on the same box.  There is no CPU fallback: without a GPU this fails."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP, REPEATS = 3, 20


def gpu_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def copy_rate():
    import torch
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t = gpu_ms(lambda: dst.copy_(src))
    return 2 * (1 << 30) / (t["median_ms"] * 1e-3)


def time_scene(style, T, res, rate):
    import numpy as np
    import torch
    from texir_code_amd import _lib, scene as S, synth
    sc0 = synth.make_scene(T, tex_res=64, style=style)
    sc = S.Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], np.zeros((2, 2, 3), np.float32), device=0)
    L = _lib.lib()
    nb = ctypes.c_int64()
    _lib.check(L.texir_texel_gbuffer_workspace_bytes(sc.h, res, res, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    pos, nrm = torch.empty(res, res, 3, device="cuda"), torch.empty(res, res, 3, device="cuda")
    prim, bary = torch.empty(res, res, dtype=torch.int32, device="cuda"), torch.empty(res, res, 2, device="cuda")
    p = _lib.ptr
    out = {"triangles": T, "atlas": res, "workspace_bytes": int(nb.value)}
    for name, ids in (("pos_nrm", False), ("pos_nrm_prim_bary", True)):
        call = lambda: _lib.check(L.texir_texel_gbuffer(sc.h, res, res, 0, 1e-2, p(pos), p(nrm), p(prim) if ids else None, p(bary) if ids else None, p(ws),
                                                        _lib.stream_ptr()))
        e = gpu_ms(call)
        e["min_bytes"] = res * res * (24 + (12 if ids else 0))
        e["share_of_copy_rate"] = round(e["min_bytes"] / (e["median_ms"] * 1e-3) / rate, 4)
        out[name] = e
    out["covered_texels"] = int((prim >= 0).sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-stage", action="store_true", help="skip tools/stage_time.py (the three routes' texel_gbuffer phases inside the IrrT stage)")
    ap.add_argument("--stage-workload", default="c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texel_raster.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("texel_raster_time: needs a GPU (nothing is measured on a CPU)")
    rate = copy_rate()
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "copy_rate_TBs": round(rate / 1e12, 3)}
    out["c4"] = time_scene("room", 1000000, 4096, rate)
    out["house"] = time_scene("house", 1000000, 4096, rate)
    if not a.no_stage:
        import stage_time
        e2e = stage_time.run(a.stage_workload, do_mat=False, pano_flow=True, raster=True)
        out["stage"] = {"workload": a.stage_workload, "texel_gbuffer_phase_s": e2e["texel_gbuffer_phase_s"],
                        "irrt_total_s": {k: e2e[k]["total_s"] for k in ("irrt", "irrt_pano_gather", "irrt_raster")},
                        "phases_s": {k: e2e[k]["phases_s"] for k in ("irrt", "irrt_pano_gather", "irrt_raster")}}
        ph = out["stage"]["texel_gbuffer_phase_s"]
        out["stage"]["raster_beats_file_and_pano"] = bool(ph["irrt_raster"] < ph["irrt"] and ph["irrt_raster"] < ph["irrt_pano_gather"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
