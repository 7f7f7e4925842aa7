"""GPU-box tests of what the scaling run depends on: the RCCL code path is executed on hardware, `bench.py --gpus N`
really starts N ranks (or refuses), and BASELINE configs[3] / [4] run at full mesh/texture size (C4: 4096^2 texels, 1 M triangles;
C5: 2 M-triangle joint NIrF -> IrT -> Mat walk-through at reduced spp)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2

pytestmark = pytest.mark.gpu


def _run(cmd, timeout=900, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=e)


def test_rccl_process_group_world_of_one(tmp_path):
    """backend "nccl" (= RCCL on ROCm) initialises and all-reduces on this box -- the calls bench.py / exp_runner make at N > 1,
    through the same helpers (dist_util.assemble_sum / reduce_texture_grads)"""
    code = (
        "import os, torch, torch.distributed as dist\n"
        "from texir_code_amd import dist_util\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', device_id=torch.device('cuda', 0))\n"
        "t = torch.arange(1 << 20, device='cuda', dtype=torch.float32)\n"
        "dist.all_reduce(t)\n"
        "dist.barrier()\n"
        "assert float(t[12345]) == 12345.0 and dist.get_world_size() == 1 and dist.get_backend() == 'nccl'\n"
        "dist_util.assemble_sum(t)\n"
        "p = torch.nn.Parameter(torch.zeros(64, 64, 3, device='cuda')); p.grad = torch.ones_like(p)\n"
        "dist_util.reduce_texture_grads([p])\n"
        "torch.cuda.synchronize(); dist.destroy_process_group(); print('rccl ok')\n")
    r = _run([sys.executable, "-c", code], env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0",
                                                "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stderr[-2000:]


def test_bench_gpus_flag_starts_ranks_or_refuses():
    """`python bench.py --gpus N` (the driver's command shape, no launcher): with fewer than N devices it must fail loudly instead of
    printing an n_gpus: 1 line; with enough devices rank 0 prints n_gpus: N measured over RCCL"""
    n_dev = torch.cuda.device_count()
    want = 2
    r = _run([sys.executable, "bench.py", "--gpus", str(want), "--workload", "tiny", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-mat"])
    if n_dev < want:
        assert r.returncode != 0 and "ranks requested" in (r.stderr + r.stdout) and '"n_gpus"' not in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    else:
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["n_gpus"] == want and line["value"] > 0
    # a launcher that started a different number of ranks than --gpus says is refused too
    r = _run([sys.executable, "bench.py", "--gpus", "1", "--workload", "tiny", "--no-cpu", "--no-mat"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def _line_and_full(r, full_path):
    """the ONE printed line (what the driver parses: <= 3 KB, contract keys) and the full record it names"""
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 3072, (len(lines), [len(x) for x in lines])
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "full"):
        assert k in line, k
    assert set(line["config"]) == {"workload", "parallelism"} and line["full"] == full_path
    full = json.load(open(full_path))
    assert full["value"] == line["value"] and full["n_gpus"] == line["n_gpus"]
    return line, full


def test_plain_bench_is_the_headline_only_and_dumps_its_last_step(tmp_path):
    """a plain run (no --full) prints the contract keys and none of the side legs; --dump-outputs writes the texture the last timed step computed:
    the same in two runs, and the same as one direct launch over the workload's valid texels"""
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = _run([sys.executable, "bench.py", "--gpus", "1", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["metric"] == "IrT generation throughput" and line["unit"] == "Mrays/s" and line["value"] > 0 and line["higher_is_better"] is True
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["full"] is None
        assert not {"roofline", "cpu_baseline", "material_step", "projected_speedup", "extra_mrays_s", "e2e_s"} & set(line), sorted(line)
        assert os.listdir(str(d)) == ["irradiance.npy"]
        dumps.append(np.load(str(d / "irradiance.npy")))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (128 * 128, 3) and float(np.abs(dumps[0]).max()) > 0
    assert rel_l2(dumps[1], dumps[0]) < 1e-6
    sys.path.insert(0, ROOT)
    import bench
    from texir_code_amd import scene as S, dist_util
    sc0, pos, nrm, valid, shift, res, spp = bench.make_workload("tiny")
    sc = S.Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], sc0["hdr"])
    ids = dist_util.morton_order(torch.nonzero(torch.from_numpy(valid.reshape(-1)) > 0)[:, 0].to(torch.int32), res).cuda()
    d = lambda a: torch.from_numpy(a).cuda()
    irr = sc.irt_generate(d(pos).reshape(-1, 3), d(nrm).reshape(-1, 3), d(shift), spp, "uniform", texel_ids=ids)
    assert rel_l2(dumps[0], irr.cpu().numpy()) < 1e-6


def test_bench_two_ranks_on_one_gpu_over_gloo(tmp_path):
    """the N > 1 bench path end to end (block-cyclic shards, all_reduce assembly, max-over-ranks timing, one JSON line from rank 0) with
    two ranks sharing this GPU over gloo; the assembled texture's throughput line must carry n_gpus: 2"""
    fp_ = str(tmp_path / "full.json")
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541",
              "bench.py", "--gpus", "2", "--workload", "tiny", "--steps", "1", "--warmup", "1", "--full", "--no-cpu",
              "--mat", "--mat-steps", "4", "--mat-res", "512", "--mat-cube", "32"],
             env={"TEXIR_DIST_BACKEND": "gloo", "TEXIR_BENCH_FULL": fp_})
    assert r.returncode == 0, r.stderr[-2000:]
    line, d = _line_and_full(r, fp_)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    # the printed line's per-rank block: kernel time of every rank, the assembly check, the bytes one step's collective moves, which backend ran (rccl_ranks is the
    # world size under nccl = RCCL, None under this test's gloo)
    lr = line["ranks"]
    assert lr["assembled_ok"] is True and len(lr["kernel_ms"]) == 2 and lr["backend"] == "gloo" and lr["rccl_ranks"] is None
    assert lr["collective_bytes_per_step"] == 12 * 12417          # 12 B per valid texel of the tiny workload (one all_gather of the compacted values)
    assert line["material_step"]["mat_shard"] == "pixel" and line["material_step_view_mode"]["mat_shard"] == "view"
    # rank 0 re-traced a sample of both ranks' texel blocks alone: the all-reduced texture must hold exactly those values
    assert d["ranks"]["assembled_ok"] is True and len(d["ranks"]["kernel_ms"]) == 2 and d["ranks"]["kernel_ms_max"] >= d["ranks"]["kernel_ms_min"] > 0
    fp = d["ranks"]["footprint_per_rank"]
    assert fp["replicated_scene_bytes"] > 0 and fp["irt_scratch_bytes"] >= 0 and fp["texel_gbuffers_bytes"] > 0
    # the material legs of the N > 1 line, both shardings: `material_step` = the trainer's default, pixel mode -- one view per step, two small
    # all_gathers of per-pixel data, every rank on the same trajectory; `material_step_view_mode` = one view per rank per step, texture gradients summed
    m = d["material_step"]
    P = 6 * 32 * 32
    assert m["mat_shard"] == "pixel" and m["views_per_step"] == 1 and m["ms"] > 0 and m["ranks_agree_on_every_loss"] is True
    assert m["collective_bytes_per_step"] == 2 * (P // 2) * (12 + 16)               # rgb [P_r,3] + (d albedo, d roughness) [P_r,4], gathered from 2 ranks
    v = d["material_step_view_mode"]
    assert v["mat_shard"] == "view" and v["views_per_step"] == 2 and v["ms"] > 0 and abs(v["ms_per_view"] - v["ms"] / 2) < 2e-3
    assert v["collective_bytes_per_step"] > m["collective_bytes_per_step"]


def test_bench_eight_ranks_on_one_gpu_over_gloo_c2_shape(tmp_path):
    """the driver's 8-GPU command shape on the one GPU there is: 8 ranks over gloo trace the 8 block-cyclic shards of a c2-shaped workload (200 k triangles,
    2048^2 texels) at 64 spp, assemble them through the all_gather, and rank 0's re-trace of sampled blocks of every rank must equal the assembled texture"""
    r = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", "29561",
              "bench.py", "--gpus", "8", "--workload", "c2", "--spp", "64", "--steps", "1", "--warmup", "1", "--full", "--no-cpu", "--no-mat"],
             timeout=1500, env={"TEXIR_DIST_BACKEND": "gloo", "TEXIR_BENCH_FULL": str(tmp_path / "full8.json")})
    assert r.returncode == 0, r.stderr[-2000:]
    line, d = _line_and_full(r, str(tmp_path / "full8.json"))
    assert d["n_gpus"] == 8 and d["ranks"]["assembled_ok"] is True and len(d["ranks"]["kernel_ms"]) == 8
    # the compact N = 8 line: per-rank kernel times, the assembly check and the collective's bytes are IN the printed line
    lr = line["ranks"]
    assert lr["assembled_ok"] is True and len(lr["kernel_ms"]) == 8 and min(lr["kernel_ms"]) > 0 and lr["collective_bytes_per_step"] > 0 and lr["backend"] == "gloo"
    assert "8" in line["config"]["parallelism"] and line["scaling"] == "strong"


def test_pixel_sharded_material_step_is_the_single_gpu_step_bit_for_bit(tmp_path):
    """VERDICT r3 #7a / weak #8.  train.mat_shard = pixel on several ranks (sharded_step.ShardedMatStep: the specular trace and its backward split by
    pixels, the texture side replicated, two small all_gathers per step, three hipGraphs per step) against the single-GPU recorded step
    (graph_step.GraphedMatStep): stages 1 and 2, five steps each over two views at 1024^2 textures -- the textures must be IDENTICAL BITS, for one
    rank, for two ranks (gloo, sharing this GPU), through hipGraphs and eagerly; and the graph path must really have been active"""
    w = os.path.join(ROOT, "tests", "sharded_worker.py")
    env = {"TEXIR_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    runs = {"single": [sys.executable, w, "single", str(tmp_path / "single.npz")],
            "sharded1": [sys.executable, w, "sharded", str(tmp_path / "sharded1.npz")],
            "sharded2": [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29547",
                         w, "sharded", str(tmp_path / "sharded2.npz")],
            "sharded2_eager": [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29549",
                               w, "sharded", str(tmp_path / "sharded2_eager.npz"), "eager"]}
    out = {}
    for name, cmd in runs.items():
        r = _run(cmd, timeout=900, env=env)
        assert r.returncode == 0, (name, r.stderr[-3000:])
        out[name] = np.load(str(tmp_path / ("%s.npz" % name)))
    ref = out["single"]
    assert float(np.abs(ref["a2"] - ref["a1"]).max()) > 1e-3 and float(np.abs(ref["r1"] - 0.35).max()) > 0          # the steps moved the textures
    for name in ("sharded1", "sharded2", "sharded2_eager"):
        o = out[name]
        assert int(o["world"][0]) == (1 if name == "sharded1" else 2)
        assert int(o["graphs"][0]) == 1, name                      # (graphs recorded in the graph runs, none in the eager run: the worker checks both)
        for k in ("a1", "r1", "a2", "r2"):
            assert np.array_equal(o[k], ref[k]), (name, k, float(np.abs(o[k] - ref[k]).max()))
        assert np.array_equal(o["losses"], ref["losses"]), name


@pytest.fixture(scope="module")
def c4_workload():
    """BASELINE.json configs[3] at full size: 1 M triangles, 4096^2 texels, 4096^2 radiance texture"""
    sys.path.insert(0, ROOT)
    import bench
    from texir_code_amd import scene as S, dist_util
    sc0, pos, nrm, valid, shift, res, spp = bench.make_workload("c4")
    sc = S.Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], sc0["hdr"])
    ids = torch.nonzero(torch.from_numpy(valid.reshape(-1)) > 0)[:, 0].to(torch.int32)
    ids = dist_util.morton_order(ids, res).cuda()
    d = lambda a: torch.from_numpy(a).cuda()
    return sc0, sc, d(pos).reshape(-1, 3), d(nrm).reshape(-1, 3), d(shift), ids, valid


def test_full_size_c4_properties(c4_workload):
    """configs[3] (the bench's own workload: 4096^2 texels / 12.5 M valid, 1 M triangles, 4k^2 texture) at reduced spp for the
    O(spp) checks and at the full 2048 spp for determinism + the 8-way shard union: finiteness, seams zero, determinism, exact
    linearity, superposition, union of the 8 block-cyclic rank shards == the single-rank texture bit for bit"""
    from texir_code_amd import dist_util
    sc0, sc, pos, nrm, shift, ids, valid = c4_workload
    v = torch.from_numpy(valid.reshape(-1) > 0).cuda()
    hdr = torch.from_numpy(sc0["hdr"]).cuda()
    N = 256
    base, st = sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids, stats=True)
    assert int(st[0]) == ids.numel() * N                                     # every ray traced
    assert torch.isfinite(base).all() and bool((base[~v] == 0).all()) and float(base[v].min()) >= 0
    sc.set_texture(hdr * 4.0)
    assert torch.equal(sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids), base * 4.0)
    A = hdr.clone()
    A[: hdr.shape[0] // 2] = 0
    sc.set_texture(A)
    ia = sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids)
    sc.set_texture(hdr - A)
    ib = sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids)
    assert rel_l2((ia + ib).cpu().numpy(), base.cpu().numpy()) < 1e-6
    sc.set_texture(torch.full_like(hdr, 0.5))
    const = sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids)[v]
    assert abs(float(const.mean()) - math.pi * 0.5) < 5e-3
    sc.set_texture(hdr)
    del ia, ib, A, const
    # full 2048 spp: two identical launches, then the 8-rank partition of the SCALE run
    N = 2048
    full = sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids)
    assert torch.equal(full, sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=ids))
    acc = torch.zeros_like(full)
    for r in range(8):
        part = dist_util.shard_block_cyclic(ids, r, 8, 4096)
        sc.irt_generate(pos, nrm, shift, N, "uniform", texel_ids=part, out=acc)
    assert torch.equal(acc, full)
    assert rel_l2(full.cpu().numpy(), base.cpu().numpy()) < 0.2               # 256 vs 2048 spp: same integral up to the 256-spp Monte-Carlo noise (measured 0.11)
    # parity at the headline configuration itself: 300 random valid texels of the full 2048-spp texture against the C oracle (its own
    # canonical BVH2 over the same 1 M triangles, same shifts) -- 614 400 rays of CPU work
    from oracle import oracle as O
    rng = np.random.default_rng(4)
    pick = np.sort(rng.choice(np.argwhere(valid.reshape(-1) > 0)[:, 0], 300, replace=False))
    osc = O.Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], sc0["hdr"])
    tp = torch.from_numpy(pick).cuda()
    ref = osc.irt_generate(pos[tp].cpu().numpy(), nrm[tp].cpu().numpy(), None, shift[tp].cpu().numpy(), N, "uniform", tracer="bvh")
    got = full[tp].cpu().numpy()
    e = rel_l2(got, ref)
    print("c4 at 2048 spp, 300 texels vs oracle: rel-L2 %.2e" % e)
    assert e < 1e-3 and e < 1e-4, e


def test_c5_joint_pipeline_smoke():
    """configs[4]: NIrF -> IrT -> pad -> Mat on the 2 M-triangle mesh (tools/run_c5.py), reduced spp / steps"""
    r = _run([sys.executable, "tools/run_c5.py", "--tris", "2000000", "--res", "2048", "--spp", "128", "--nirf-steps", "5", "--mat-steps", "5"], timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["scene"]["triangles"] == 2000000
    assert d["nirf"]["gt_Mrays_s"] > 0 and math.isfinite(d["nirf"]["final_loss"])
    assert d["irt"]["Mrays_s"] > 0 and d["material_step"]["ms"] > 0
