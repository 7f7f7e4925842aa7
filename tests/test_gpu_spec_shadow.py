"""spec_shadow_kernel (csrc/specshadow.hip) behind texir_spec_shadow, Scene.spec_shadow, irtlight.add_view(lost_spec=) and the evaluation model's
test.spec_shadows, on the golden box (12 triangles) and room (20 k).

  1. intervals     every case of spec_shadow_cases inside its float64 reference, stats inside its counts, unlisted pixels untouched, the prefilter off: the
                   same bits and the same blocked count.  S in 1, 16, 24, 64, 100; lists of 1 .. 200 pixels; TEXIR_SPEC_LPP in 1, 4, 16; a grid of two
                   blocks; M in 1, 2, 3, 4, 5, 8 (every MMAX); Kb / J in (0, 0), (1, 0), (0, 1), (8, 8), (3, 2), (2, 1);
  2. full shadow   pixels inside a ball body, and pixels inside a closed box instance: lost IS spec_render(irr = 0, albedo = 0), bit for bit;
  3. no shadow     bodies and objects no accepted hit lies behind, Kb = J = 0, a zero mask: exactly +0; nothing met: stats[0] == 0;
  4. one sample    S = 1: lost == where(blocked, L w, 0) bit for bit;
  5. restatement   general S: against spec_shadow_f32 fed the device's own hits and occlusion answers;
  6. order, union  0 <= lost <= the specular term; superset >= subset; {body, instance} covering the same rays; J = 0 == eight instances that block nothing;
  7. purity        a second run, a shuffled list, duplicates and ids outside [0, P), a side stream, a graph replayed after bodies, matrices and sets moved;
  8. errors        every refused argument raises with the header's text and writes nothing;
  9. poses         host poses and the device [J,12] form: the same bits;
 10. model         test.spec_shadows = true equals add_view of direct calls; absent or false: the bits and files of before.
"""
import os

import numpy as np
import pytest
import torch

import irt_shadow_mesh_cases as MC
import spec_cases as SC
import spec_shadow_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = C.SENTINEL
_SC, _OCC, _DEV = {}, {}, {}


def scene_of(tx, geo):
    if geo.name not in _SC:
        _SC[geo.name] = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
    return _SC[geo.name]


def occluder_of(tx, name):
    if name not in _OCC:
        g = MC.occluder(name)
        _OCC[name] = tx.Scene.occluder(g.verts, g.tris)
    return _OCC[name]


def dev_inputs(c):
    key = (c.geo.name, c.P)
    if key not in _DEV:
        _DEV[key] = tuple(torch.from_numpy(a).cuda() for a in (c.pos, c.nrm, c.rough, c.shift))
    return _DEV[key]


def masks_of(sets):
    return torch.from_numpy(np.array(sets, np.uint32).view(np.int32)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def env_of(monkeypatch, c):
    """the case's switches, and proof that the library read them"""
    from texir_code_amd import _lib
    if c.lpp:
        monkeypatch.setenv("TEXIR_SPEC_LPP", str(c.lpp))
        assert _lib.env_switch("TEXIR_SPEC_LPP") == c.lpp
    if c.grid_cap:
        monkeypatch.setenv("TEXIR_SPEC_GRID_CAP", str(c.grid_cap))
        assert _lib.env_switch("TEXIR_SPEC_GRID_CAP") == c.grid_cap


def shadow(tx, c, ids=None, w2o=None, bodies=None, sets=None, **kw):
    """the call on the case's DEVICE records, matrices (world-to-object, the first J of the buffer) and raw masks"""
    pos, nrm, rough, shift = dev_inputs(c)
    sets = c.sets if sets is None else sets
    out = torch.full((len(sets), c.P, 3), SENTINEL, device="cuda")
    ids = torch.from_numpy(c.ids).cuda() if ids is None else ids
    w2o = torch.from_numpy(np.ascontiguousarray(c.w2o)).cuda() if w2o is None else w2o
    bodies = torch.from_numpy(np.ascontiguousarray(c.bodies)).cuda() if bodies is None else bodies
    got, st = scene_of(tx, c.geo).spec_shadow(pos, nrm, rough, shift, c.cam, c.S, bodies=bodies, occluders=[occluder_of(tx, n) for n in c.occ], instances=c.inst,
                                              poses=w2o, sets=masks_of(sets), texel_ids=ids, clamp_eps=c.ceps, out=out, stats=True, **kw)
    assert got is out
    return out.cpu().numpy(), st.cpu().numpy()


def spec_term(tx, c, rows=None):
    """spec_render(irr = 0, albedo = 0) on the case's listed pixels -> [len(listed), 3]"""
    L = torch.from_numpy(c.listed if rows is None else rows).cuda()
    pos, nrm, rough, shift = (t[L].contiguous() for t in dev_inputs(c))
    z = torch.zeros((len(L), 3), device="cuda")
    return tx.spec_render(scene_of(tx, c.geo), nrm, z, rough, pos, z, torch.from_numpy(c.cam).cuda(), shift, c.S, clamp_eps=c.ceps).cpu().numpy()


def variant(c, tag, **kw):
    """the case with some arguments changed (no cache)"""
    a = dict(ids=c.ids, S=c.S, bodies=c.buf, occ=c.occ, inst=c.inst_buf, sets=c.sets, Kb=c.Kb, J=c.J, ceps=c.ceps, lpp=c.lpp, w2o=c.w2o_buf)
    a.update(kw)
    ids, S = a.pop("ids"), a.pop("S")
    return C.Case(c.name.split(":", 1)[1] + "_" + tag, c.geo, c.pos, c.nrm, c.rough, c.shift, c.cam, ids, S, **a)


# ---- 1. intervals ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.GPU_CASES)
def test_every_case_inside_its_float64_reference(tx, monkeypatch, name):
    c = C.case(name)
    env_of(monkeypatch, c)
    lost, st = shadow(tx, c)
    print("spec_shadow %s: stats %s, reference counts %s, caps %s" % (name, st.tolist(), c.ref().counts(), c.ref().caps()))
    worst = C.check(c, lost, st, SENTINEL, "gpu")
    print("spec_shadow %s: worst share of the interval %.4f" % (name, worst))
    assert worst <= 1.0
    off, st_off = shadow(tx, c, prefilter=False)
    assert np.array_equal(bits(lost), bits(off)), "the prefilter changes a bit"
    assert st_off[2] == st[2] and st_off[0] >= st[0]
    valid_inst = int(sum(np.isfinite(w).all() for w in c.w2o))
    if valid_inst:
        assert st_off[0] == len(c.ids) * c.S, "prefilter off: every sample of a listed pixel counts as met"


# ---- 2. full shadow = the specular term --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["in_ball", "in_cube"])
@pytest.mark.parametrize("S,lpp", [(1, 0), (16, 0), (24, 0), (100, 0), (16, 4), (24, 4)])
def test_a_full_shadow_is_the_specular_term_bit_for_bit(tx, monkeypatch, name, S, lpp):
    c = variant(C.case(name), "S%d_lpp%d" % (S, lpp), S=S, lpp=lpp)
    env_of(monkeypatch, c)
    r = c.ref()
    sel = r.all_blocked(0)
    assert sel.sum() >= (2 if S == 1 else 6), int(sel.sum())
    lost, st = shadow(tx, c)
    want = spec_term(tx, c)
    a, b = bits(lost[0][r.pix[sel]]), bits(want[sel])
    assert np.array_equal(a, b), "%d of %d pixels differ" % ((a != b).any(1).sum(), int(sel.sum()))
    assert (want[sel] > 0).any()
    print("%s S %d lpp %d: %d pixels equal the specular term bit for bit; stats %s" % (name, S, lpp, int(sel.sum()), st.tolist()))


# ---- 3. no shadow ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_nothing_in_front_gives_plus_zero(tx):
    c = C.case("far")                                                          # met by rays, never in front of an accepted hit
    lost, st = shadow(tx, c)
    assert not bits(lost[:, c.listed]).any() and st[0] > 0 and st[2] == 0
    c0 = C.case("none")                                                        # Kb = J = 0
    lost, st = shadow(tx, c0)
    assert not bits(lost[:, c0.listed]).any() and st.tolist() == [0, 0, 0]
    # a record the rule refuses and a speck of an object far outside the room: the reference finds no ray that may meet anything (a lobe's rays can leave
    # a floor pixel downwards, so "under the floor" is not such a place here)
    specks = variant(c, "specks", bodies=C.SH.eight_records()[2:3], Kb=1, occ=["cube"], inst=[0],
                     w2o=MC.to_world_to_object(np.stack([MC.pose((300.0, 400.0, -500.0), scale=0.01)])), J=1, sets=[0x101, 0x1, 0x100])
    assert specks.ref().meet_maybe.sum() == 0
    lost, st = shadow(tx, specks)
    assert not bits(lost[:, specks.listed]).any() and st.tolist() == [0, 0, 0]
    assert (lost[:, np.setdiff1d(np.arange(c.P), specks.listed)] == SENTINEL).all()
    full = C.case("in_ball")                                                   # a zero mask, and one that is zero once the bits that name nothing are gone
    lost, st = shadow(tx, full, sets=[0, 0xFFFFFF00 & ~0x100 | 0xFE, full.sets[0]])
    assert not bits(lost[:2, full.listed]).any() and np.abs(lost[2, full.listed]).any() and st[2] > 0


# ---- 4. one sample -----------------------------------------------------------------------------------------------------------------------------------------------------

class DeviceTrace:
    """the device's own answers for restated rays: the scene's closest hits with their radiance, an occluder's any-hit answer inside (0, t_far) -- taken
    per ray from its closest hit, which texir_trace_occluded's rule states equal to test_occlusions(t_near = 0, t_far) bit for bit"""

    def __init__(self, tx, c):
        self.tx, self.c = tx, c

    def scene(self, org, dir):
        rad, t, pid, _ = scene_of(self.tx, self.c.geo).trace_shade(org, dir, return_hits=True)
        return t.cpu().numpy(), pid.cpu().numpy(), rad.cpu().numpy()

    def occluded(self, j, org, dir, t_far):
        occ = occluder_of(self.tx, self.c.occ[self.c.inst_buf[j]])
        _, t, pid, _ = occ.trace_shade(org, dir, return_hits=True)
        t, pid = t.cpu().numpy(), pid.cpu().numpy()
        anyhit = occ.test_occlusions(org, dir).cpu().numpy()
        assert np.array_equal(anyhit, pid >= 0)
        with np.errstate(invalid="ignore"):
            return (pid >= 0) & (t > 0) & (t < t_far)


@pytest.mark.parametrize("name", ["s1_p63", "s1_p64", "s1_p65", "s1_p200"])
def test_one_sample_is_L_times_w_where_blocked(tx, name):
    """S = 1: lost == where(blocked, L w, 0), bit for bit, on every listed pixel of every set.
    blocked   the float32 body restatement OR the occluder's own answer on the restated object-space ray, against t_s of the restated ray from trace_shade
              (spec_shadow_f32 on the device's answers); the reference is certain of every one of these decisions (spec_shadow_cases.choose).
    w         the device's own: spec_forward on given lighting = 1 at S = 1 returns exactly w (one fused multiply-add of 1 * w onto +0, then / 1).
    L         the radiance of the sample's hit along the DEVICE'S OWN direction: what spec_forward's traced form keeps per sample (its Ls workspace, the
              hit shader's output for the ray spec_sample gave).  The numpy chain's direction differs from the device's in its last bit on some pixels
              (sincosf), so trace_shade on the RESTATED ray cannot give the device's L bit for bit on all of them; its radiance is held, on every
              pixel, inside the float64 reference's interval of the pixel's specular term (the chain's bound of l carried through trace_cases.RayRef's
              radiance bound, times the interval of w, plus the accumulation term), and where it reproduces the device's radiance it is the same number"""
    c = C.case(name)
    r = c.ref()
    assert c.S == 1 and not r.uncertain.any() and not r.left.any()
    lost, st = shadow(tx, c)
    tr = DeviceTrace(tx, c)
    L = torch.from_numpy(c.listed).cuda()
    pos, nrm, rough, shift = (t[L].contiguous() for t in dev_inputs(c))
    z = torch.zeros((len(L), 3), device="cuda")
    cam = torch.from_numpy(c.cam).cuda()
    term, Ls, _ = tx.spec_forward_raw(scene_of(tx, c.geo), nrm, z, rough, pos, z, cam, shift, 1, c.ceps)
    w = tx.spec_render(None, nrm, z, rough, pos, z, cam, shift, 1, clamp_eps=c.ceps, lighting=torch.ones((len(L), 1, 3), device="cuda")).cpu().numpy()
    assert (w == w[:, :1]).all() and np.isfinite(w).all()
    L_dev = Ls.reshape(len(L), 3).cpu().numpy()
    prod = (L_dev * w).astype(np.float32)
    assert np.array_equal(bits(prod), bits(term.cpu().numpy())), "spec_forward's own term is not its L times its w"
    n_blocked = 0
    for m, mask in enumerate(c.masks()):
        one = variant(c, "set%d" % m, sets=[mask])
        blocked = np.abs(C.spec_shadow_f32(one, "no_weight", trace=tr)[0][0][c.listed]).sum(1) > 0       # L alone: a blocked sample with w = 0 still shows
        n_blocked += int(blocked.sum())
        want = np.where(blocked[:, None], prod, np.float32(0))
        a, b = bits(lost[m][c.listed]), bits(want)
        assert np.array_equal(a, b), "set %d: %d of %d pixels differ" % (m, (a != b).any(1).sum(), len(c.listed))
    assert n_blocked > 0
    # trace_shade on the restated ray: every pixel inside the reference's interval of the specular term
    _, l = C.chain_f32(c)
    t, pid, rad = tr.scene(c.pos[c.listed], l)
    got = (rad * w).astype(np.float64)
    nr = SC.n_acc(1, 0)
    lo, hi = r.spec_lo[:, 0], r.spec_hi[:, 0]
    acc = C.KF * (nr * C.U * np.maximum(np.abs(lo), np.abs(hi)) + (nr + 4) * C.TINY)
    bad = ~((got >= lo - acc) & (got <= hi + acc))
    assert not bad.any(), "%d values of L(restated ray) w outside the reference's interval, first at pixel %d" % (int(bad.sum()), int(c.listed[np.argwhere(bad)[0, 0]]))
    same_ray = (bits(rad) == bits(L_dev)).all(1)
    assert np.array_equal(bits((rad * w).astype(np.float32))[same_ray], bits(prod)[same_ray])
    print("%s: %d pixels, %d blocked (set by set); trace_shade on the restated ray gives the device's radiance bit for bit on %.0f %%" % (name, len(c.listed), n_blocked,
                                                                                                                                        100 * same_ray.mean()))


# ---- 5. restatement ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s16_p5", "s24_eight", "s100", "lpp4_s24", "twice", "overlap", "room_person"])
def test_general_S_against_the_float32_restatement_on_the_devices_own_hits(tx, monkeypatch, name):
    c = C.case(name)
    env_of(monkeypatch, c)
    lost, st = shadow(tx, c)
    f32, st32 = C.spec_shadow_f32(c, trace=DeviceTrace(tx, c))
    assert C.check(c, f32, None, SENTINEL, "restatement on device hits") <= 1.0
    r = c.ref()
    nr = SC.n_acc(c.S, c.lpp)
    for m in range(c.M):
        # both lie inside the pixel's interval: they differ by at most its width (the samples' own intervals and the accumulation term)
        width = ((r.hi[m] - r.lo[m]).sum(1) + 2 * C.KF * (nr * C.U * np.maximum(np.abs(r.lo[m]), np.abs(r.hi[m])).sum(1) + (nr + 4) * C.TINY)) / c.S
        d = np.abs(lost[m][r.pix].astype(np.float64) - f32[m][r.pix].astype(np.float64))
        assert (d <= width).all(), "set %d: %d values further apart than the interval is wide" % (m, int((d > width).sum()))
        same = (bits(lost[m][r.pix]) == bits(f32[m][r.pix])).all(1).mean()
        print("%s set %d: %.0f %% of the pixels equal the restatement bit for bit" % (name, m, 100 * same))
    assert st[2] == st32[2] and st[0] == st32[0], (st.tolist(), st32.tolist())


# ---- 6. order and union ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_order_and_union(tx):
    c = C.case("s24_eight")
    sets = [0, 0x1, 0x3, 0x23, 0x123, 0x1F23, 0xFFFF, 0xFF00]                   # a chain of supersets, then the instances alone
    lost, st = shadow(tx, c, sets=sets)
    term = spec_term(tx, c)
    got = lost[:, c.listed]
    assert (got >= 0).all() and not np.signbit(got).any() and (got <= term[None]).all(), "0 <= lost <= the specular term"
    for a in range(6):
        assert (got[a + 1] >= got[a]).all(), "set %d is a superset of set %d" % (a + 1, a)
    assert (got[6] >= got[7]).all() and np.abs(got[6]).any() and np.abs(got[7]).any()
    # a body and an instance covering the same rays: where one fully covers the other the union equals it alone
    # the icosphere (radius 0.5, scaled by 0.6: every vertex 0.3 from the centre) lies inside the ball of radius 0.5 around the same centre: a ray that
    # enters the icosphere before the scene's hit has entered the ball before, so the ball covers it and the union is the ball alone
    o = C.case("overlap")
    lost, _ = shadow(tx, o)                                                    # sets {ball, ico}, {ball}, {ico}
    g = lost[:, o.listed]
    assert (g[0] >= g[2]).all() and (g[1] > g[2]).any() and np.abs(g[2]).any()
    assert np.array_equal(bits(g[0]), bits(g[1])), "the union of the ball and the icosphere inside it is the ball alone"
    cov = variant(C.case("in_ball"), "cov", occ=["cube"], inst=[0], w2o=MC.to_world_to_object(np.stack([MC.enclosing_cube()])), J=1, sets=[0x1, 0x100, 0x101])
    lost, _ = shadow(tx, cov)
    g = lost[:, cov.listed]
    assert np.array_equal(bits(g[0]), bits(g[2])) and np.abs(g[0]).any(), "inside the ball: the ball alone is the union"
    # bodies only, J = 0, against the same call with eight instances that block nothing
    b = variant(c, "bodies", occ=[], inst=[], w2o=np.zeros((0, 12), np.float32), J=0, sets=[0xFF, 0x21])
    base, st0 = shadow(tx, b)
    under = MC.to_world_to_object(np.stack([MC.pose((-3.0 - k, -3.0, -3.0)) for k in range(8)]))
    e = variant(c, "under", occ=["cube"], inst=[0] * 8, w2o=under, J=8, sets=[0xFFFF, 0xFF21])
    got8, st8 = shadow(tx, e)
    assert np.array_equal(bits(base), bits(got8)) and st8[2] == st0[2] and st8[0] >= st0[0]


# ---- 7. purity -----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_result_is_a_pure_function_of_the_inputs(tx):
    c = C.case("s16_grid")
    base, st = shadow(tx, c)
    ids = torch.from_numpy(c.ids).cuda()
    n = len(c.ids)
    again, st2 = shadow(tx, c)
    assert np.array_equal(bits(base), bits(again)) and st.tolist() == st2.tolist(), "second run"
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    assert np.array_equal(bits(base), bits(shadow(tx, c, ids[perm])[0])), "permuted list"
    extra = torch.tensor([-3, c.P, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    mixed, st3 = shadow(tx, c, torch.cat([ids[:50], extra, ids, ids[:40]]))
    assert np.array_equal(bits(base), bits(mixed)), "duplicates and ids outside [0, P)"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side, _ = shadow(tx, c)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(base), bits(on_side)), "side stream"
    pos, nrm, rough, shift = dev_inputs(c)
    occ = [occluder_of(tx, n_) for n_ in c.occ]
    pairs = scene_of(tx, c.geo).spec_shadow(pos, nrm, rough, shift, c.cam, c.S, bodies=c.bodies, occluders=occ, instances=c.inst, poses=c.poses,
                                            sets=[([0, 1, 2], [0, 1]), ([], [0, 1])], texel_ids=ids, clamp_eps=c.ceps)
    assert np.array_equal(bits(base[:, c.listed]), bits(pairs.cpu().numpy()[:, c.listed])), "sets as index pairs, host poses"
    dflt = scene_of(tx, c.geo).spec_shadow(pos, nrm, rough, shift, c.cam, c.S, bodies=c.bodies, occluders=occ, instances=c.inst, poses=c.poses, texel_ids=ids,
                                           clamp_eps=c.ceps)
    assert tuple(dflt.shape) == (1, c.P, 3) and np.array_equal(bits(dflt.cpu().numpy()[0, c.listed]), bits(base[0, c.listed])), "default: one set of everything"


def test_a_replayed_graph_sees_the_bodies_matrices_and_sets_the_device_holds_then(tx):
    import ctypes as Ct
    from texir_code_amd import _lib
    c = C.case("s16_p5")
    L = _lib.lib()
    sc = scene_of(tx, c.geo)
    pos, nrm, rough, shift = dev_inputs(c)
    cam = torch.from_numpy(c.cam).cuda()
    ids = torch.from_numpy(c.ids).cuda()
    n, P, M, guard = len(c.ids), c.P, c.M, 64
    occ = [occluder_of(tx, n_) for n_ in c.occ]
    handles = (Ct.c_void_p * len(occ))(*[o.h for o in occ])
    inst = np.array(c.inst, np.int32)
    w2o = torch.from_numpy(np.ascontiguousarray(c.w2o)).cuda()
    bodies = torch.from_numpy(np.ascontiguousarray(c.bodies)).cuda()
    masks = masks_of(c.sets)
    out = torch.full((M * P * 3 + guard,), SENTINEL, device="cuda")
    stats = torch.zeros(3, dtype=torch.int64, device="cuda")
    base, st0 = shadow(tx, c)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                                 # the single call on one stream: no parallel branches
            _lib.check(L.texir_spec_shadow(sc.h, _lib.ptr(nrm), _lib.ptr(rough), _lib.ptr(pos), _lib.ptr(cam), _lib.ptr(shift), _lib.ptr(ids), n, P, c.S, c.ceps,
                                           _lib.ptr(bodies), c.Kb, Ct.cast(handles, Ct.c_void_p), len(occ), _lib.ptr(inst), _lib.ptr(w2o), c.J, _lib.ptr(masks), M, 0,
                                           _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)

    def replay(want, want_st, what):
        out.fill_(SENTINEL)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(want), bits(out[:M * P * 3].reshape(M, P, 3).cpu().numpy())), what
        assert stats.cpu().tolist() == want_st.tolist(), what
        assert (out[M * P * 3:] == SENTINEL).all(), "guard words"
    replay(base, st0, "graph replay")
    replay(base, st0, "second graph replay")
    moved_w = MC.to_world_to_object(np.stack([C.TABLE_AT(4.0, 3.0, 50.0), C.ICO_AT(4.0, 1.25, 3.0, 10.0, 1.2)]))
    moved_b = np.stack([C.BACK_PANEL(), C.SH.ball([5.5, 0.5, 2.0], 0.6), C.COVER_BALL()])
    moved_s = np.array([s ^ 0x0303 for s in c.sets], np.uint32)
    w2o.copy_(torch.from_numpy(moved_w))
    bodies.copy_(torch.from_numpy(moved_b))
    masks.copy_(torch.from_numpy(moved_s.view(np.int32)))
    fresh, st1 = shadow(tx, c, w2o=torch.from_numpy(moved_w).cuda(), bodies=torch.from_numpy(moved_b).cuda(), sets=[int(s) for s in moved_s])
    assert not np.array_equal(bits(fresh), bits(base))
    replay(fresh, st1, "graph replay after the bodies, matrices and sets were overwritten on the device")


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise_and_write_nothing(tx, monkeypatch):
    import ctypes as Ct
    from texir_code_amd import _lib
    c = C.case("s16_p5")
    sc = scene_of(tx, c.geo)
    pos, nrm, rough, shift = dev_inputs(c)
    ids = torch.from_numpy(c.ids).cuda()
    occ = [occluder_of(tx, n_) for n_ in c.occ]
    out = torch.full((2, c.P, 3), SENTINEL, device="cuda")
    two = [0xFFFF, 0x1]

    def call(**kw):
        a = dict(bodies=c.bodies, occluders=occ, instances=c.inst, poses=c.poses, sets=two, texel_ids=ids, out=out)
        a.update(kw)
        return sc.spec_shadow(pos, nrm, rough, shift, c.cam, a.pop("S", 16), **a)
    with pytest.raises(_lib.TexirError, match="Kb must be in 0..8, got 9"):
        call(bodies=np.tile(c.bodies[:1], (9, 1)))
    with pytest.raises(_lib.TexirError, match="Q must be in 0..8, got 9"):
        call(occluders=[occ[0]] * 9)
    with pytest.raises(_lib.TexirError, match="J must be in 0..8, got 9"):
        call(instances=[0] * 9, poses=np.tile(MC.pose()[None], (9, 1, 1)))
    with pytest.raises(_lib.TexirError, match="M must be in 1..8, got 9"):
        call(sets=[1] * 9, out=None)
    with pytest.raises(_lib.TexirError, match="M must be in 1..8, got 0"):
        call(sets=[], out=None)
    with pytest.raises(_lib.TexirError, match=r"inst_obj\[1\] = 2 names no occluder \(Q = 2\)"):
        call(instances=[0, 2])
    with pytest.raises(_lib.TexirError, match=r"inst_obj\[0\] = -1 names no occluder"):
        call(instances=[-1, 1])
    for bad in (0, -16):
        with pytest.raises(_lib.TexirError, match="S must be in 1..65536"):
            call(S=bad)
    with pytest.raises(_lib.TexirError, match="clamp_eps must be finite and > 0"):
        call(clamp_eps=0.0)
    with pytest.raises(ValueError, match="pose 1 is singular"):
        call(poses=np.stack([c.poses[0], np.zeros((3, 4))]))
    with pytest.raises(ValueError, match="2 instances, 1 poses"):
        call(poses=c.poses[:1])
    with pytest.raises(ValueError, match="occluders must be Scene handles"):
        call(occluders=[occ[0], None])
    with pytest.raises(ValueError, match="names body 3: the call has 3 bodies"):
        call(sets=[([3], [])])
    with pytest.raises(ValueError, match="names instance 2: the call has 2 instances"):
        call(sets=[([0], [2])])
    with pytest.raises(ValueError, match="bodies must be"):
        call(bodies=np.zeros((2, 15), np.float32))
    with pytest.raises(ValueError, match="out must be"):
        call(out=torch.zeros((3, c.P, 3), device="cuda"))
    assert call(texel_ids=ids[:0]) is out                                      # an empty list never reaches the library
    L = _lib.lib()
    cam = torch.from_numpy(c.cam).cuda()
    w2o, masks, inst = torch.from_numpy(np.ascontiguousarray(c.w2o)).cuda(), masks_of(two), np.array(c.inst, np.int32)
    bodies = torch.from_numpy(np.ascontiguousarray(c.bodies)).cuda()

    def raw(n_ids, s=sc, handles=occ, **null):
        hs = (Ct.c_void_p * len(handles))(*[o.h for o in handles])
        p = lambda name, t: None if name in null else _lib.ptr(t)
        return L.texir_spec_shadow(s.h, p("normal", nrm), p("rough", rough), p("points", pos), p("cam", cam), p("shift", shift), _lib.ptr(ids), n_ids, c.P, 16, 1e-14,
                                   p("bodies", bodies), 3, Ct.cast(hs, Ct.c_void_p), 2, _lib.ptr(inst), p("w2o", w2o), 2, p("sets", masks), 2, 0, p("out", out), None,
                                   _lib.stream_ptr())
    for name, text in (("normal", "null argument"), ("rough", "null argument"), ("points", "null argument"), ("cam", "null argument"), ("shift", "null argument"),
                       ("out", "null argument"), ("bodies", "bodies is null"), ("sets", "sets is null"), ("w2o", "inst_world_to_obj is null")):
        with pytest.raises(_lib.TexirError, match=text):
            _lib.check(raw(5, **{name: True}))
    _lib.check(raw(0))                                                        # a non-null empty list writes nothing
    monkeypatch.setenv("TEXIR_BVH_WIDTH", "2")
    binary = tx.Scene(c.geo.verts, c.geo.tris, c.geo.tri_uvs, c.geo.hdr)
    g = MC.occluder("ico")
    binary_occ = tx.Scene.occluder(g.verts, g.tris)
    monkeypatch.delenv("TEXIR_BVH_WIDTH")
    with pytest.raises(_lib.TexirError, match="the scene has no 4-wide tree"):
        _lib.check(raw(5, binary))
    with pytest.raises(_lib.TexirError, match=r"occluders\[1\] has no 4-wide tree"):
        _lib.check(raw(5, sc, [occ[0], binary_occ]))
    if torch.cuda.device_count() > 1:
        other = tx.Scene.occluder(g.verts, g.tris, device=1)
        with pytest.raises(_lib.TexirError, match=r"occluders\[1\] lives on device 1, the scene on device 0"):
            _lib.check(raw(5, sc, [occ[0], other]))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- 9. poses ------------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_host_poses_and_the_device_form_give_the_same_bits(tx):
    c = C.case("s100")
    base, _ = shadow(tx, c)                                                    # the device [J,12] world-to-object tensor
    pos, nrm, rough, shift = dev_inputs(c)
    out = torch.full((c.M, c.P, 3), SENTINEL, device="cuda")
    occ = [occluder_of(tx, n_) for n_ in c.occ]
    scene_of(tx, c.geo).spec_shadow(pos, nrm, rough, shift, c.cam, c.S, bodies=c.bodies, occluders=occ, instances=c.inst, poses=c.poses, sets=list(c.sets),
                                    texel_ids=torch.from_numpy(c.ids).cuda(), clamp_eps=c.ceps, out=out)
    assert np.array_equal(bits(base), bits(out.cpu().numpy())) and np.abs(base[:, c.listed]).any()


# ---- 10. the evaluation model ------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_evaluation_model_takes_the_specular_shadow_from_the_view(tx, tmp_path):
    """render() with test.spec_shadows = true is add_view(lost_spec=) of direct calls; with the key absent or false it returns the bits it returned before
    (Editing and View write render()'s pixels and nothing else of the model: the same bits are the same files), and draws nothing more from the CPU generator"""
    import json
    from texir_code_amd import irtlight
    from texir_code_amd.tester import lit_model as LM, test_model as TM
    c = C.case("room_person")
    pick = c.listed[:64]
    shape = (1, 8, 8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    rng = np.random.default_rng(23)
    normal, points = dev(c.nrm[pick].reshape(shape + (3,))), dev(c.pos[pick].reshape(shape + (3,)))
    albedo, irr = dev(rng.random(shape + (3,), dtype=np.float32)), dev(rng.random(shape + (3,), dtype=np.float32))
    rough, cam = dev(c.rough[pick].reshape(shape + (1,))), dev(c.cam)
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [3.0, 2.5, 2.0], "a": [2.0, 0.0, 0.0], "b": [0.0, 0.0, 2.0], "colour": [20, 18, 15]},
                                         {"kind": "sphere", "c": [4.0, 1.25, 3.0], "r": 0.5}]}))
    g = MC.occluder("table")
    obj = tmp_path / "table.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in q) for q in g.verts) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in g.tris))
    spec = [{"obj": str(obj), "pose": {"translate": [3.0, 0.0, 2.5], "rotate_deg": [0, 20, 0], "scale": 1.0}}]
    m = LM.MaterialModel.__new__(LM.MaterialModel)
    torch.nn.Module.__init__(m)
    m.scene = scene_of(tx, c.geo)
    m.device, m.sample_l, m.sample_type, m.relighting = m.scene.device, [16, 16], ["uniform", "importance"], False
    torch.manual_seed(5)
    plain = m.render(normal, albedo, rough, points, cam, irr)
    m.test_lights, m.light_samples = LM.load_test_lights(str(js), m.device), 16
    m.test_objects = LM.load_test_objects(spec, m.test_lights, m.device)
    torch.manual_seed(5)
    absent = m.render(normal, albedo, rough, points, cam, irr)                # the attribute itself is absent: a model built before the key existed
    state = torch.get_rng_state()
    m.spec_shadows = LM.spec_shadow_setting({}, m.test_lights)
    assert m.spec_shadows is False
    torch.manual_seed(5)
    off = m.render(normal, albedo, rough, points, cam, irr)
    m.spec_shadows = LM.spec_shadow_setting({"test.spec_shadows": True}, m.test_lights)
    torch.manual_seed(5)
    on = m.render(normal, albedo, rough, points, cam, irr)
    assert torch.equal(torch.get_rng_state(), state), "the specular shadow drew from the CPU generator"
    torch.manual_seed(5)
    shift_s = torch.rand(64, 1, 2).reshape(64, 2).cuda()                      # the pixels' own specular shift
    records, colours = m.test_lights
    flat = (points.reshape(-1, 3), normal.reshape(-1, 3))
    kw = m.test_objects
    F = m.scene.irt_lights(*flat, shift_s, records, 16, **kw)
    R = m.scene.spec_lights(*flat, rough.reshape(-1), shift_s, cam, records, 16, clamp_eps=TM.TINY_NUMBER, **kw)
    want_off = irtlight.add_view(plain["rgb"].reshape(-1, 3), albedo.reshape(-1, 3), F, R, colours).reshape(shape + (3,))
    assert torch.equal(absent["rgb"], want_off) and torch.equal(off["rgb"], want_off), "absent or false: render() is what it was"
    lost = m.scene.spec_shadow(*flat, rough.reshape(-1), shift_s, cam, 16, bodies=records, clamp_eps=TM.TINY_NUMBER, **kw)
    assert tuple(lost.shape) == (1, 64, 3) and (lost > 0).any()
    want_on = irtlight.add_view(plain["rgb"].reshape(-1, 3), albedo.reshape(-1, 3), F, R, colours, lost_spec=lost[0]).reshape(shape + (3,))
    assert torch.equal(on["rgb"], want_on) and not torch.equal(on["rgb"], off["rgb"]) and (on["rgb"] <= off["rgb"]).all()
    for k in ("albedo", "normal", "position"):
        assert torch.equal(on[k], plain[k])
