"""Wave-uniform node steps (device_common.h node_step4: the float node read by three scalar loads, one body per ray octant) against the per-lane
path of a scene built without float nodes (TEXIR_UNIFORM_FLOAT=0).  Both prune with the same conservative boxes, so every hit and every
irradiance bit must agree.  The rays come in 64-ray bundles that share an origin and a direction octant, so that whole waves take the uniform
path, in each of the eight octants."""
import numpy as np
import pytest
import torch


def _scenes(golden, monkeypatch):
    from texir_code_amd import scene as S
    g = golden("irt_room.npz")
    sc = S.Scene(g["verts"], g["tris"], g["tri_uvs"], g["hdr"])
    monkeypatch.setenv("TEXIR_UNIFORM_FLOAT", "0")
    sc_q = S.Scene(g["verts"], g["tris"], g["tri_uvs"], g["hdr"])
    monkeypatch.delenv("TEXIR_UNIFORM_FLOAT")
    assert sc_q.info()["node_bytes"] < sc.info()["node_bytes"]          # (only the default scene carries the float nodes)
    return g, sc, sc_q


def _bundles(g, per_octant=48, seed=7):
    """per octant, `per_octant` bundles of 64 rays: one origin (a texel point lifted off its surface), directions in a narrow cone whose
    components all keep the octant's signs"""
    rng = np.random.default_rng(seed)
    valid = np.argwhere(g["valid"].reshape(-1) > 0)[:, 0]
    pos, nrm = g["pos"].reshape(-1, 3), g["nrm"].reshape(-1, 3)
    org, dirs = [], []
    for octant in range(8):
        sign = np.array([-1.0 if octant & (1 << a) else 1.0 for a in range(3)])
        for _ in range(per_octant):
            t = rng.choice(valid)
            o = pos[t] + 1e-3 * nrm[t]
            d0 = rng.uniform(0.25, 1.0, 3)
            d = d0[None, :] + rng.uniform(-0.05, 0.05, (64, 3))
            org.append(np.repeat(o[None, :], 64, 0))
            dirs.append(np.abs(d) * sign)
    return np.concatenate(org).astype(np.float32), np.concatenate(dirs).astype(np.float32)


@pytest.mark.gpu
def test_uniform_steps_match_per_lane_steps_in_every_octant(golden, monkeypatch):
    g, sc, sc_q = _scenes(golden, monkeypatch)
    org, dirs = _bundles(g)
    a = [x.cpu().numpy() for x in sc.trace_shade(org, dirs, return_hits=True)]
    b = [x.cpu().numpy() for x in sc_q.trace_shade(org, dirs, return_hits=True)]
    torch.cuda.synchronize()
    rad_a, t_a, pid_a, uv_a = a
    rad_b, t_b, pid_b, uv_b = b
    assert (pid_a >= 0).mean() > 0.5                                       # (the bundles mostly hit: the comparison is not vacuous)
    for k in range(8):                                                     # every octant's body is exercised
        assert (pid_a[k * 48 * 64:(k + 1) * 48 * 64] >= 0).any()
    assert np.array_equal(pid_a, pid_b)
    assert np.array_equal(t_a.view(np.uint32), t_b.view(np.uint32))
    assert np.array_equal(uv_a.view(np.uint32), uv_b.view(np.uint32))
    assert np.array_equal(rad_a.view(np.uint32), rad_b.view(np.uint32))


@pytest.mark.gpu
def test_uniform_steps_match_per_lane_steps_irradiance(golden, monkeypatch):
    g, sc, sc_q = _scenes(golden, monkeypatch)
    v = np.argwhere(g["valid"].reshape(-1) > 0)[:, 0]
    ids = torch.from_numpy(v.astype(np.int32)).cuda()
    args = (torch.from_numpy(g["pos"]), torch.from_numpy(g["nrm"]), torch.from_numpy(g["shift"]), 128, "cosine")
    a = sc.irt_generate(*args, texel_ids=ids).cpu().numpy()
    b = sc_q.irt_generate(*args, texel_ids=ids).cpu().numpy()
    assert np.array_equal(a[v].view(np.uint32), b[v].view(np.uint32))
