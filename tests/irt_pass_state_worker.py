"""Worker of tests/test_gpu_irt_pass_state.py: every case of that file under ONE setting of TEXIR_IRT_SPECIALISE, which the library reads when it loads --
so each setting gets a process of its own.
    TEXIR_IRT_SPECIALISE=0|1 TEXIR_IRT_TEXELS_PER_WAVE=64 python tests/irt_pass_state_worker.py out.npz
Scene and texel list are irt_specialised_worker.problem()'s.  Writes, per case, the irradiance of the listed texels ("irr/<case>") and the instantiation the
launcher reports ("variant/<case>").  Case names: <what>_<instantiation>_<N>, instantiation = uniform | cosine | estimator (the cosine estimator of
diffuse_irradiance)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from irt_specialised_worker import N_LISTED, problem          # noqa: E402

INSTANTIATIONS = ("uniform", "cosine", "estimator")
SAMPLES = (1, 2, 16, 512, 2048)       # one part ... 32 parts; 1 and 2048 = the largest and (with the bench's N) a small exponent of 1 / N
LISTS = (5, 64)                       # a partial group alone; exactly one full group
N_EDGE = 8                            # the first texels of the list take the edge shifts below
LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))         # the largest float32 below 1
EDGE_SHIFTS = [(0.0, 0.0), (LAST, LAST), (0.0, LAST), (LAST, 0.0), (0.5, 0.0), (0.0, 0.5), (LAST, 0.5), (0.5, LAST)]


def main():
    out = sys.argv[1]
    assert os.environ.get("TEXIR_IRT_SPECIALISE") in ("0", "1") and os.environ.get("TEXIR_IRT_TEXELS_PER_WAVE") == "64"
    torch.cuda.set_device(0)
    from texir_code_amd import _lib, scene as S
    assert _lib.env_switch("TEXIR_IRT_SPECIALISE") == int(os.environ["TEXIR_IRT_SPECIALISE"])
    assert _lib.env_switch("TEXIR_IRT_MIN_PART_CELLS") == 8 and _lib.env_switch("TEXIR_IRT_LOG2PARTS") == -1 and _lib.env_switch("TEXIR_IRT_REFILL") == 0
    assert _lib.env_switch("TEXIR_IRT_GRID_CAP") == 0
    sc0, born, pos, nrm, shift, ids = problem()
    packed = S.Scene(sc0["verts"], sc0["tris"], sc0["tri_uvs"], born, device=0)
    assert packed.texture_layout() == 4
    edge = shift.copy()
    edge[ids[:N_EDGE]] = np.array(EDGE_SHIFTS, np.float32)
    assert edge[ids[1], 0] < 1.0 and np.float32(edge[ids[1], 0]) == np.float32(LAST)
    d_pos, d_nrm, d_shift, d_edge, d_ids = (torch.from_numpy(a).cuda() for a in (pos, nrm, shift, edge, ids))
    res = {}

    def generate(case, inst, N, sh, listed=N_LISTED):
        l = d_ids[:listed]
        lid = l.long()
        if inst == "estimator":           # the listed texels as the points of diffuse_irradiance (no id list)
            res["irr/" + case] = S.diffuse_irradiance(packed, d_pos[lid], d_nrm[lid], sh[lid], N, "cosine").cpu().numpy()
        else:
            irr = torch.full((pos.shape[0], 3), 7.0, device="cuda")
            packed.irt_generate(d_pos, d_nrm, sh, N, inst, texel_ids=l, out=irr)
            unlisted = torch.ones(pos.shape[0], dtype=torch.bool, device="cuda")
            unlisted[lid] = False
            assert bool((irr[unlisted] == 7.0).all()), case           # nothing but the listed texels is written
            res["irr/" + case] = irr[lid].cpu().numpy()
        res["variant/" + case] = np.array(packed.irt_kernel_variant(listed, N, "cosine" if inst == "estimator" else inst, cosine_estimator=inst == "estimator"))

    for inst in INSTANTIATIONS:
        for N in SAMPLES:
            generate("all_%s_%d" % (inst, N), inst, N, d_shift)
        generate("again_%s_64" % inst, inst, 64, d_shift)
        generate("all_%s_64" % inst, inst, 64, d_shift)                # the same call a second time
        for n in LISTS:
            generate("list%d_%s_64" % (n, inst), inst, 64, d_shift, listed=n)
        for N in (64, 2048):                                           # shifts 0 and 1 - 2^-24: the cell offsets wrap
            generate("edge_%s_%d" % (inst, N), inst, N, d_edge)
    # one block of four waves: every wave runs many chunks in turn
    os.environ["TEXIR_IRT_GRID_CAP"] = "1"
    _lib.reload_env()
    assert _lib.env_switch("TEXIR_IRT_GRID_CAP") == 1
    for inst in INSTANTIATIONS:
        generate("oneblock_%s_64" % inst, inst, 64, d_shift)
    del os.environ["TEXIR_IRT_GRID_CAP"]
    _lib.reload_env()
    torch.cuda.synchronize()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
