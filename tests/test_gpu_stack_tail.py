"""The stack tail of a traversal step (csrc/device_common.h trace_core: pop_lds -- the top entry read whole, the culled entries behind it examined two per
LDS round trip) against the float64 reference of tests/trace_cases.py: every ray by the per-ray rule (TC.check_hits), every texel inside the sum of its
samples' intervals (IrtRef.check) -- never one kernel form against another.  The cases are the small ones of test_gpu_trace_kernels.py (their caps are proved by
test_trace_ref_cpu.py), chosen for what the stack does in them:
    lists of 1 / 63 / 65 / 130 texels at N = 64, 70 texels at N = 512, one and 64 texels per wave           ragged waves; a lane's stack runs empty (the one-entry pair, the empty-stack read)
    TEXIR_IRT_REFILL=32                                                                                      irt_stream_kernel: a lane restarts on an empty stack mid-wave
    TEXIR_MAX_LEAF=1                                                                                         a deeper tree: stacks reach past the 10 LDS entries and come back
    rays: room, scan, 3000 stacked triangles (every child of a node is hit: three pushes per level)          long runs of culled entries after the first hit
    the specular lighting Ls on the deeper tree                                                              spec kernels share trace_core
That the cases do what they are chosen for is ASSERTED with the kernel's own counters (stats[6]: entries dropped by culling, stats[7]: pushes and pops through
the private overflow part), from the counting instantiations of the same kernels, whose textures go through the same per-texel check.

MEASURED on an MI355X (26 tests, 6 s, all passing): every IrT case culls (stats[6] > 0); the two TEXIR_MAX_LEAF=1 cases at N = 512 push two entries past the
LDS part and pop them again (stats[7] = 4), every other case stays inside it; worst error / bound 0.084 on the rays (room_random), 0.076 on the specular
lighting; the IrT cases as in test_gpu_trace_kernels.py."""
import numpy as np
import pytest
import torch

import trace_cases as TC
import test_gpu_trace_kernels as K

pytestmark = pytest.mark.gpu

N64 = ("room", 130, 64, "uniform", False, None)
N512 = ("room", 70, 512, "uniform", False, None)
# (key, rows of the list, environment)
IRT = ([(N64, n, {"TEXIR_IRT_TEXELS_PER_WAVE": pw}) for n in (1, 63, 65, 130) for pw in ("1", "64")]
       + [(N512, 70, {"TEXIR_IRT_TEXELS_PER_WAVE": pw}) for pw in ("1", "64")]
       + [(k, k[1], {"TEXIR_IRT_TEXELS_PER_WAVE": "64", "TEXIR_IRT_REFILL": "32"}) for k in (N64, N512)]
       + [(k, k[1], {"TEXIR_IRT_TEXELS_PER_WAVE": pw, "TEXIR_MAX_LEAF": "1"}) for k in (N64, N512) for pw in ("1", "64")])
IRT_IDS = ["%dx%d_%s" % (n, k[2], "+".join("%s=%s" % kv for kv in e.items()).replace("TEXIR_", "")) for k, n, e in IRT]
_STATS = {}


def counted(tx, monkeypatch, i):
    """case i through the shipped kernel AND through its counting instantiation, both against the reference; returns the counters of the second"""
    if i not in _STATS:
        key, n, env = IRT[i]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = TC.irt_case(*key)
        rows = slice(0, n)
        sc = K.gpu_scene(tx, c.geo)
        form, parts = K.irt_run(tx, c, sc=sc, rows=rows, family="stack_tail", what=IRT_IDS[i])
        use = c.ids[rows]
        tid = torch.from_numpy(use.astype(np.int32)).cuda()
        irr, st = sc.irt_generate(torch.from_numpy(c.pos), torch.from_numpy(c.nrm), torch.from_numpy(c.shift), c.N, c.mode, texel_ids=tid, stats=True)
        c.ref().check(irr.cpu().numpy()[use], form, parts, "stack_tail", "%s counted %s/%d" % (IRT_IDS[i], form, parts), rows=rows)
        st = st.cpu().numpy()
        assert st[0] == n * c.N and st[1] > 0 and st[2] > 0
        _STATS[i] = st[:8].copy()
    return _STATS[i]


@pytest.mark.parametrize("i", range(len(IRT)), ids=IRT_IDS)
def test_irt_per_texel(tx, monkeypatch, i):
    st = counted(tx, monkeypatch, i)
    print("stats", IRT_IDS[i], st.tolist())
    assert st[6] > 0                                  # (every case culls: a texel's hemisphere always holds rays whose first hit hides pushed children)


def test_cases_reach_the_overflow_part_and_cull(tx, monkeypatch):
    """coverage by the counters: entries are culled everywhere, the single-texel lists ran (a wave whose other lanes' stacks are empty from the start), and at
    least one case pushed beyond the LDS part of the stack and popped back into it -- the pops crossed the boundary between pop and pop_lds"""
    st = np.stack([counted(tx, monkeypatch, i) for i in range(len(IRT))])
    assert (st[:, 6] > 0).all()
    single = [i for i, (k, n, e) in enumerate(IRT) if n == 1]
    assert len(single) == 2 and all(st[i, 0] == 64 for i in single)
    print("overflow pushes + pops per case", dict(zip(IRT_IDS, st[:, 7].tolist())))
    assert (st[:, 7] > 0).any()
    assert (st[:, 7] % 2 == 0).all()                  # (every entry pushed into the overflow part is popped from it again)


@pytest.mark.parametrize("leaf", [None, "1"])
@pytest.mark.parametrize("name", ["room_random", "room_hemisphere", "scan_random", "patho_stack"])
def test_closest_hits_per_ray(tx, monkeypatch, name, leaf):
    if leaf:
        monkeypatch.setenv("TEXIR_MAX_LEAF", leaf)
    c = K.ray_case(name)
    t, pid, uv, rad = K.trace(K.gpu_scene(tx, c.geo), c)
    TC.check_hits(c.ref(), t, pid, uv, rad, "stack_tail", "%s leaf=%s" % (name, leaf))


def test_specular_lighting_on_the_deeper_tree(tx, monkeypatch):
    monkeypatch.setenv("TEXIR_MAX_LEAF", "1")
    K.test_specular_lighting_per_sample(tx)
