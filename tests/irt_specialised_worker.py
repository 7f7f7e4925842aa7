"""Worker of tests/test_gpu_irt_specialised.py: every case of that file under ONE setting of TEXIR_IRT_SPECIALISE, which the library reads when it loads --
so each setting gets a process of its own.
    TEXIR_IRT_SPECIALISE=0|1 TEXIR_IRT_TEXELS_PER_WAVE=64 python tests/irt_specialised_worker.py out.npz
Writes, per case, the irradiance of the listed texels ("irr/<case>"), the kernel form and the instantiation the launcher reports ("form/<case>",
"variant/<case>") and, for the counting case, the first four counters ("stats/<case>")."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LISTED = 209                      # three full 64-texel groups and a partial one of 17: dead lanes in the last wave
ZERO_NORMAL, AXIS_NORMAL = 5, 70    # positions in the list of the two texels that take make_frame's special arms (first and second group)


def problem():
    """a ~2 000-triangle room, its texture as an RGBE file holds it and as the generator's floats, and 209 listed texels of a 32 x 32 texel G-buffer"""
    from texir_code_amd import synth
    sc0 = synth.make_scene(2000, tex_res=128)
    pos, nrm, valid = synth.make_texel_gbuffer(sc0, 32)
    shift = synth.make_shifts(32 * 32)
    pos, nrm = pos.reshape(-1, 3).copy(), nrm.reshape(-1, 3).copy()
    ids = np.argwhere(valid.reshape(-1) > 0)[:, 0]
    ids = ids[np.linspace(0, len(ids) - 1, N_LISTED).astype(np.int64)].astype(np.int32)          # spread over all the room's charts
    assert len(np.unique(ids)) == N_LISTED
    nrm[ids[ZERO_NORMAL]] = 0.0                                                                  # |n| = 0: the frame divides by 1e-6
    nrm[ids[AXIS_NORMAL]] = np.array([0.995, 0.05, -0.03], np.float32)                           # |n.x| > 0.99: the frame's other axis
    return sc0, synth.rgbe_born(sc0["hdr"]), pos, nrm, shift, ids


def main():
    out = sys.argv[1]
    assert os.environ.get("TEXIR_IRT_SPECIALISE") in ("0", "1") and os.environ.get("TEXIR_IRT_TEXELS_PER_WAVE") == "64"
    torch.cuda.set_device(0)
    from texir_code_amd import _lib, scene as S
    assert _lib.env_switch("TEXIR_IRT_SPECIALISE") == int(os.environ["TEXIR_IRT_SPECIALISE"])
    # the default plan: N = 64 is cut into 8 parts (partial sums + combine kernel), N = 8 is one part (written by the kernel itself)
    assert _lib.env_switch("TEXIR_IRT_MIN_PART_CELLS") == 8 and _lib.env_switch("TEXIR_IRT_LOG2PARTS") == -1 and _lib.env_switch("TEXIR_IRT_REFILL") == 0
    sc0, born, pos, nrm, shift, ids = problem()
    geo = (sc0["verts"], sc0["tris"], sc0["tri_uvs"])
    packed = S.Scene(*geo, born, device=0)
    floats = S.Scene(*geo, sc0["hdr"], device=0)
    os.environ["TEXIR_UNIFORM_FLOAT"] = "0"
    _lib.reload_env()
    quantised = S.Scene(*geo, born, device=0)                 # no float node copy: every node step per lane
    del os.environ["TEXIR_UNIFORM_FLOAT"]
    _lib.reload_env()
    assert packed.texture_layout() == 4 and floats.texture_layout() == 2 and quantised.texture_layout() == 4
    assert quantised.info()["node_bytes"] < packed.info()["node_bytes"]
    d_pos, d_nrm, d_shift, d_ids = (torch.from_numpy(a).cuda() for a in (pos, nrm, shift, ids))
    lid = d_ids.long()
    res = {}

    def generate(case, sc, N, mode, stats=False):
        irr = torch.full((pos.shape[0], 3), 7.0, device="cuda")
        r = sc.irt_generate(d_pos, d_nrm, d_shift, N, mode, texel_ids=d_ids, out=irr, stats=stats)
        if stats:
            res["stats/" + case] = r[1][:4].cpu().numpy()
        unlisted = torch.ones(pos.shape[0], dtype=torch.bool, device="cuda")
        unlisted[lid] = False
        assert bool((irr[unlisted] == 7.0).all()), case           # nothing but the listed texels is written
        res["irr/" + case] = irr[lid].cpu().numpy()
        res["form/" + case] = np.array(sc.irt_kernel_name(N_LISTED, N))
        res["variant/" + case] = np.array(sc.irt_kernel_variant(N_LISTED, N, mode))

    for N in (64, 8):                                             # 8 parts + combine; one part, written directly
        for mode in ("uniform", "cosine"):
            generate("packed_%s_%d" % (mode, N), packed, N, mode)
        # the cosine estimator: the listed texels as the points of diffuse_irradiance (no id list)
        E = S.diffuse_irradiance(packed, d_pos[lid], d_nrm[lid], d_shift[lid], N, "cosine")
        res["irr/packed_estimator_%d" % N] = E.cpu().numpy()
        res["form/packed_estimator_%d" % N] = np.array(packed.irt_kernel_name(N_LISTED, N))
        res["variant/packed_estimator_%d" % N] = np.array(packed.irt_kernel_variant(N_LISTED, N, "cosine", cosine_estimator=True))
    generate("packed_uniform_48", packed, 48, "uniform")         # not a power of two
    generate("floats_uniform_64", floats, 64, "uniform")         # texture layout 2
    generate("quantised_uniform_64", quantised, 64, "uniform")   # no float nodes
    generate("counted_uniform_64", packed, 64, "uniform", stats=True)
    torch.cuda.synchronize()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
