"""Times of the pad + denoise step between the stages (csrc/texpost.hip, texir_code_amd/texpost.py) on one GPU, in one process, beside the parent route
of the same step (tools.padding_texture on the CPU, tools.denoise_atrous on the torch device) on the same input on the same box.

    python tools/texpost_time.py [--res 4096] [--workload seeded|c4] [--no-cpu] [--no-stage] [--out profiles/texpost.json]

Input: the seeded atlas-like image of tests/texpost_cases.py's recipe at --res^2 with cell = 64 (guides: normals from the gradient of the mask's noise
field, positions from the texel coordinates); --workload c4: the IrT stage's output and texel G-buffers of the c4 scene (tools/stage_time.py's assets).
Every GPU figure is the median of 20 HIP-event times after 3 warm-up rounds; per a-trous pass the two tap forms (LDS tile / global loads) are timed
separately through TEXIR_ATROUS_LDS_PASSES.  `min_bytes` is what each must move at least, from shapes; `share_of_8TBs` is that over the time over the
8 TB/s HBM peak -- a reported figure, not a target (the pad's walk and the filter's 25 taps are served by the caches).  There is no CPU fallback: without
a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_BYTES_S = 8.0e12
WARMUP, REPEATS = 3, 20


def seeded_input(res, cell=64):
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(666)
    z = torch.rand(1, 1, res // cell + 2, res // cell + 2, generator=g)
    field = F.interpolate(z, size=(res, res), mode="bicubic", align_corners=False)[0, 0]
    valid = field > 0.42
    img = (torch.rand(res, res, 3, generator=torch.Generator().manual_seed(1)) + 0.25) * valid[..., None]
    gy, gx = torch.gradient(field * (res / cell))
    nrm = torch.stack([-gx, -gy, torch.ones_like(field)], -1)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    yy, xx = torch.meshgrid(torch.arange(res, dtype=torch.float32), torch.arange(res, dtype=torch.float32), indexing="ij")
    pos = torch.stack([xx / res, yy / res, field * 0.1], -1)
    return img.contiguous(), nrm.contiguous(), pos.contiguous(), float(valid.float().mean())


def c4_input():
    """the IrT output + texel G-buffers of the c4 scene"""
    import contextlib
    import io
    import stage_time
    from texir_code_amd.trainer.generate_ir_texture import IrrTextureRunner
    root = tempfile.mkdtemp(prefix="texir_texpost_")
    _, conf_irt, _, _ = stage_time.make_assets(root, "c4")
    with contextlib.redirect_stdout(io.StringIO()):
        runner = IrrTextureRunner(conf=conf_irt, exps_folder_name="exps", expname="t", max_niters=1, gpu_index=0)
        img = runner.run()
    occ = float((img.sum(-1) != 0).float().mean())
    return img.cpu(), runner.model.normal_texture.cpu(), runner.model.position_texture.cpu(), occ, root


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


def with_bytes(entry, nbytes):
    entry["min_bytes"] = int(nbytes)
    entry["share_of_8TBs"] = round(nbytes / (entry["median_ms"] * 1e-3) / PEAK_BYTES_S, 4)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--workload", default="seeded", choices=("seeded", "c4"))
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU route (seconds per call at 4096^2)")
    ap.add_argument("--no-stage", action="store_true", help="skip tools/stage_time.py --irt-post (the irt_post phase inside the IrrT stage's wall time)")
    ap.add_argument("--stage-workload", default="c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texpost.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("texpost_time: needs a GPU (nothing is measured on a CPU)")
    from texir_code_amd import _lib, texpost, tools
    L = _lib.lib()
    root = None
    if a.workload == "c4":
        img, nrm, pos, occ, root = c4_input()
    else:
        img, nrm, pos, occ = seeded_input(a.res)
    H, W, _ = img.shape
    n = H * W
    out = {"input": "%s %dx%d, occupancy %.3f" % (a.workload, H, W, occ), "warmup": WARMUP, "repeats": REPEATS, "device": torch.cuda.get_device_name(0)}
    d_img, d_nrm, d_pos = img.cuda(), nrm.cuda(), pos.cuda()

    # ---- pad: launches only (buffers and index tables made once, as a recorded graph would hold them)
    ws = torch.empty(int(L.texir_texture_pad_workspace_bytes(H, W)), dtype=torch.uint8, device="cuda")
    d_out, d_src = torch.empty_like(d_img), torch.empty((H, W), dtype=torch.int32, device="cuda")
    rm = torch.from_numpy(texpost.reference_index_map(H)).cuda()
    cm = torch.from_numpy(texpost.reference_index_map(W)).cuda()
    p = _lib.ptr
    pad = lambda r, c: _lib.check(L.texir_texture_pad(p(d_img), H, W, 3, r, c, p(d_out), p(d_src), p(ws), _lib.stream_ptr()))
    # read the image (phase 1) + write and read the column table + read the image again and write out + src
    pad_bytes = n * (12 + 4 + 4 + 12 + 12 + 4)
    out["pad_nearest"] = with_bytes(gpu_ms(lambda: pad(None, None)), pad_bytes)
    out["pad_reference"] = with_bytes(gpu_ms(lambda: pad(p(rm), p(cm))), pad_bytes)
    padded = texpost.pad_texture(d_img, "nearest")
    assert not bool((padded.sum(-1) == 0).any())

    # ---- denoise on the padded texture, guides padded with the same sources
    _, src = texpost.pad_texture(d_img, "nearest", return_src=True)
    g_nrm, g_pos = texpost.gather_src(d_nrm, src).contiguous(), texpost.gather_src(d_pos, src).contiguous()
    tmp, res = torch.empty_like(padded), torch.empty_like(padded)
    f = __import__("ctypes").c_float

    def den(guided, iters=3):
        _lib.check(L.texir_texture_denoise(p(padded), H, W, p(g_nrm) if guided else None, p(g_pos) if guided else None, iters, f(0.5), f(0.3), f(0.25),
                                           p(tmp), p(res), _lib.stream_ptr()))

    for name, guided, per_pass in (("denoise_color", False, 24), ("denoise_guided", True, 48)):
        out[name] = with_bytes(gpu_ms(lambda: den(guided)), 3 * n * per_pass)              # per pass: read + write the colour (+ read two guides)
        forms = {}
        for lds in (0, 1, 2, 3):
            os.environ["TEXIR_ATROUS_LDS_PASSES"] = str(lds)
            _lib.reload_env()
            forms["first_%d_passes_from_lds" % lds] = gpu_ms(lambda: den(guided))["median_ms"]
        del os.environ["TEXIR_ATROUS_LDS_PASSES"]
        _lib.reload_env()
        out[name]["three_passes_ms_by_form"] = forms

    # ---- the route of the parent commit for the same step on the same box: scipy + grid_sample on the CPU, then the torch filter on the device
    # (several hundred launches; upload and download included, as its callers pay them)
    if not a.no_cpu:
        host = img.numpy()
        t0 = time.perf_counter()
        cpu_padded = tools.padding_texture(host)
        out["cpu_padding_texture_s"] = round(time.perf_counter() - t0, 3)
        tools.denoise_atrous(cpu_padded, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tools.denoise_atrous(cpu_padded, device="cuda")
        out["torch_device_denoise_atrous_s"] = round(time.perf_counter() - t0, 3)
        gpu_route = (out["pad_nearest"]["median_ms"] + out["denoise_color"]["median_ms"]) * 1e-3
        cpu_route = out["cpu_padding_texture_s"] + out["torch_device_denoise_atrous_s"]
        out["gpu_route_s"], out["cpu_route_s"], out["gpu_beats_cpu"] = round(gpu_route, 5), round(cpu_route, 3), bool(gpu_route < cpu_route)

    # ---- irt_post inside the IrrT stage's wall time
    if not a.no_stage:
        import stage_time
        e2e = stage_time.run(a.stage_workload, do_mat=False, pano_flow=False, irt_post=True)
        out["stage"] = {"workload": a.stage_workload, "irrt_total_s": e2e["irrt"]["total_s"], "irt_post_s": e2e["irrt"]["phases_s"].get("irt_post"),
                        "phases_s": e2e["irrt"]["phases_s"]}
    if root:
        import shutil
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
