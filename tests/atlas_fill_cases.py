"""The float32 restatement of the atlas fill's rule (include/texir_hip.h, texir_atlas_fill) with its mutants, the float64 reference with the header's rounding
bounds, the check of a result against it, and the seeded cases.  Shared by test_atlas_fill_ref_cpu.py (no GPU) and test_gpu_atlas_fill.py; no tests here.
K = 4 and U = 2^-24 are texture_cases'; every margin below is the header's ROUNDING BOUND times K, nothing is taken from a kernel's output.

PER (HOLE t, SOURCE s), from the float32 inputs held in float64 (c = cos_fill, r2 = max_dist^2):
  distance    dd with  e = K 5 u dd.
  range       certainly within: r2 - dd > K (5 u dd + u r2) (or r2 infinite and dd finite); certainly out: dd - r2 > the same; else undecided.
  compatible  ens = K 3 u N1;  g = ns^2 - c^2 nn_t nn_s,  eg = K (6 u N1 |ns| + u ns^2 + 9 u c^2 nn_t nn_s).
              certainly compatible: ns > ens and g > eg;   certainly incompatible: ns < -ens or g < -eg (a zero normal: N1 = 0, ns = 0, g = 0: the float32
              test computes ns = 0 exactly, and 0 > 0 fails: certainly incompatible);   else undecided.
A source CERTAINLY QUALIFIES when it is certainly compatible and certainly within.  With L = the smallest dd + e among them:
  a source is admissible iff it is not certainly incompatible, not certainly out of range and dd - e <= L;   -1 is admissible iff none certainly qualifies.
  EXACT TIES: two sources whose float32 dd (the header's sequence) are bit-identical AND whose exact dd agree tie under the rule itself: the lowest id must
  win, so the higher id is inadmissible when the lower one certainly qualifies.
The binding check of the device is bit equality with fill_f32; the float64 tier shows that fill_f32 states the rule.
"""
import numpy as np

import atlas_bake_cases as ABC
import trace_cases as TC  # noqa: F401  (atlas_bake_cases' geometry; imported so that both modules share one cache)
from texture_cases import K, U

F32, F64 = np.float32, np.float64
CAP_MULTI = ABC.CAP_MULTI
SENTINEL = (-7, -3.5)                     # (src, dist2) of unlisted texels
MUTANTS = ("no_normal", "no_range", "farthest", "tie_high", "manhattan", "unit_normals", "holes_as_sources")


class Case:
    """pos, nrm [Nt,3] f32; sources, holes: int32 lists as the caller passes them (duplicates and ids outside [0, Nt) allowed); bounds [6] f32"""

    def __init__(self, name, pos, nrm, sources, holes, cos_fill=0.5, max_dist=0.5, bounds=None):
        self.name = name
        self.pos, self.nrm = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
        self.Nt = self.pos.shape[0]
        self.sources, self.holes = np.ascontiguousarray(sources, np.int32).reshape(-1), np.ascontiguousarray(holes, np.int32).reshape(-1)
        self.cos_fill, self.max_dist = float(F32(cos_fill)), float(F32(max_dist))
        if bounds is None:
            ids = np.concatenate([self.valid_sources(), self.valid_holes()])
            p = self.pos[ids] if ids.size else np.zeros((1, 3), F32)
            bounds = np.concatenate([p.min(0), p.max(0)])
        self.bounds = np.ascontiguousarray(bounds, F32).reshape(6)
        self._ref = self._f32 = None

    def _valid(self, ids):
        ids = ids.astype(np.int64)
        return np.unique(ids[(ids >= 0) & (ids < self.Nt)])

    def valid_sources(self):
        return self._valid(self.sources)

    def valid_holes(self):
        return self._valid(self.holes)

    def with_(self, name, **kw):
        a = dict(pos=self.pos, nrm=self.nrm, sources=self.sources, holes=self.holes, cos_fill=self.cos_fill, max_dist=self.max_dist, bounds=self.bounds)
        a.update(kw)
        return Case(name, **a)

    def ref(self):
        if self._ref is None:
            self._ref = Ref(self)
        return self._ref

    def f32(self):
        """fill_f32 of the unchanged rule, computed once: (src, dist2, stats)"""
        if self._f32 is None:
            self._f32 = fill_f32(self)
        return self._f32


# ---- float32 restatement of the header's operation sequence, brute force over all hole x source pairs ----------------------------------------------------------------

def fill_f32(case, mut=None, sentinel=SENTINEL):
    """-> (src [Nt] i32, dist2 [Nt] f32, stats [2] = list entries decided, of them filled); unlisted texels hold the sentinel"""
    c = case
    src = np.full(c.Nt, sentinel[0], np.int32)
    dist2 = np.full(c.Nt, sentinel[1], F32)
    H, S = c.valid_holes(), c.valid_sources()
    if mut == "holes_as_sources":
        S = np.union1d(S, H)
    if mut == "tie_high":
        S = S[::-1]                                                        # argmin keeps the FIRST of equals: the highest id
    r2, c2 = F32(c.max_dist) * F32(c.max_dist), F32(c.cos_fill) * F32(c.cos_fill)
    pt, nt = c.pos[H], c.nrm[H]
    ps, ns_ = c.pos[S], c.nrm[S]
    win, wdd = np.full(len(H), -1, np.int64), np.zeros(len(H), F32)
    if len(S):
        with np.errstate(all="ignore"):
            nn_s = (ns_[:, 0] * ns_[:, 0] + ns_[:, 1] * ns_[:, 1]) + ns_[:, 2] * ns_[:, 2]
            for a in range(0, len(H), 256):
                p, n = pt[a:a + 256, None, :], nt[a:a + 256, None, :]
                e = ps[None] - p
                dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                ns = (n[..., 0] * ns_[None, :, 0] + n[..., 1] * ns_[None, :, 1]) + n[..., 2] * ns_[None, :, 2]
                nn_t = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
                within = dd <= r2
                compat = (ns > 0) & (ns * ns >= (c2 * nn_t) * nn_s[None])
                if mut == "no_range":
                    within = np.ones_like(within)
                if mut == "no_normal":
                    compat = np.ones_like(compat)
                if mut == "unit_normals":
                    compat = ns >= F32(c.cos_fill)
                ok = within & compat
                key = dd
                if mut == "manhattan":
                    key = (np.abs(e[..., 0]) + np.abs(e[..., 1])) + np.abs(e[..., 2])
                if mut == "farthest":
                    j = np.where(ok, key, F32(-np.inf)).argmax(1)
                else:
                    j = np.where(ok, key, F32(np.inf)).argmin(1)
                rows = np.arange(len(j))
                got = ok[rows, j]
                win[a:a + 256] = np.where(got, S[j], -1)
                wdd[a:a + 256] = np.where(got, dd[rows, j], F32(0))
    src[H], dist2[H] = win, wdd
    hl = c.holes.astype(np.int64)
    hl = hl[(hl >= 0) & (hl < c.Nt)]
    stats = np.array([len(hl), int((src[hl] >= 0).sum())], np.int64)
    return src, dist2, stats


# ---- float64 reference ------------------------------------------------------------------------------------------------------------------------------------------------

class Ref:
    def __init__(self, case):
        self.case = c = case
        self.H, self.S = H, S = c.valid_holes(), c.valid_sources()
        nH, nS = len(H), len(S)
        pt, nt = c.pos[H].astype(F64), c.nrm[H].astype(F64)
        ps, ns_ = c.pos[S].astype(F64), c.nrm[S].astype(F64)
        cf, r2 = F64(c.cos_fill), F64(c.max_dist) ** 2
        with np.errstate(all="ignore"):
            e = ps[None] - pt[:, None]
            self.dd = dd = (e * e).sum(-1)
            self.e = K * 5 * U * dd
            ns = (nt[:, None] * ns_[None]).sum(-1)
            N1 = (np.abs(nt[:, None]) * np.abs(ns_[None])).sum(-1)
            nn_t, nn_s = (nt * nt).sum(-1)[:, None], (ns_ * ns_).sum(-1)[None]
            ens = K * 3 * U * N1
            g = ns * ns - cf * cf * nn_t * nn_s
            eg = K * (6 * U * N1 * np.abs(ns) + U * ns * ns + 9 * U * cf * cf * nn_t * nn_s)
            self.compat_yes = (ns > ens) & (g > eg)
            self.compat_no = (ns < -ens) | (g < -eg) | (N1 == 0)
            if np.isinf(r2):
                self.in_yes, self.in_no = np.isfinite(dd), np.zeros((nH, nS), bool)
            else:
                er = K * (5 * U * dd + U * r2)
                self.in_yes, self.in_no = (r2 - dd > er), (dd - r2 > er)
            self.certain = self.compat_yes & self.in_yes
            self.Lbest = np.where(self.certain, dd + self.e, np.inf).min(1) if nS else np.full(nH, np.inf)
            ok = ~self.compat_no & ~self.in_no & (dd - self.e <= self.Lbest[:, None])
        # exact ties: bit-identical float32 dd and equal exact dd; the lower certainly qualifying id shuts the higher one out (S is ascending)
        e32 = c.pos[S][None] - c.pos[H][:, None]
        dd32 = (e32[..., 0] * e32[..., 0] + e32[..., 1] * e32[..., 1]) + e32[..., 2] * e32[..., 2]
        shut = np.zeros((nH, nS), bool)
        for i in range(nH):
            cand = np.nonzero(ok[i])[0]
            if len(cand) < 2:
                continue
            for a_, j in enumerate(cand):
                lower = cand[:a_]
                tw = lower[(dd32[i, lower] == dd32[i, j]) & (dd[i, lower] == dd[i, j]) & self.certain[i, lower]]
                if len(tw):
                    shut[i, j] = True
        self.ok = ok & ~shut
        self.none_ok = ~self.certain.any(1) if nS else np.ones(nH, bool)
        self.n_outcomes = self.ok.sum(1) + self.none_ok
        self.col_of = {int(s): j for j, s in enumerate(S)}

    def caps(self):
        return float((self.n_outcomes > 1).mean()) if len(self.H) else 0.0

    def stats(self):
        return {"holes": len(self.H), "sources": len(self.S), "certainly_filled": int(self.certain.any(1).sum()) if len(self.S) else 0,
                "multi": int((self.n_outcomes > 1).sum())}


def check(case, src, dist2=None, sentinel=None):
    """every listed hole: src admissible, dist2 within the bound of its exact dd (0 for -1); unlisted texels keep the sentinel -> list of failure strings"""
    ref = case.ref()
    src = np.asarray(src).reshape(-1).astype(np.int64)
    assert src.shape[0] == case.Nt
    fails = []
    for i, t in enumerate(ref.H):
        s = int(src[t])
        why = None
        if s < 0:
            if s != -1:
                why = "src %d" % s
            elif not ref.none_ok[i]:
                why = "-1 but source(s) %s certainly qualify" % ref.S[np.nonzero(ref.certain[i])[0][:4]].tolist()
            elif dist2 is not None and dist2[t] != 0:
                why = "-1 with dist2 %r" % float(dist2[t])
        elif s not in ref.col_of:
            why = "texel %d is not a listed source" % s
        else:
            j = ref.col_of[s]
            if not ref.ok[i, j]:
                why = ("source %d inadmissible (incompatible %d, out of range %d, dd %.9g +- %.3g against %.9g)"
                       % (s, ref.compat_no[i, j], ref.in_no[i, j], ref.dd[i, j], ref.e[i, j], ref.Lbest[i]))
            elif dist2 is not None and not abs(float(dist2[t]) - ref.dd[i, j]) <= ref.e[i, j]:
                why = "dist2 %.9g is not dd %.9g of source %d" % (float(dist2[t]), ref.dd[i, j], s)
        if why:
            fails.append("hole %d: %s" % (t, why))
    if sentinel is not None:
        un = np.setdiff1d(np.arange(case.Nt), ref.H)
        if un.size and not ((src[un] == sentinel[0]).all() and (dist2 is None or (np.asarray(dist2)[un] == F32(sentinel[1])).all())):
            fails.append("unlisted texels were written")
    return fails


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------------------------

_CACHE = {}
LIST_HOLES, LIST_SOURCES = (1, 63, 64, 65, 257), (1, 64, 300, 3000)
BALL_SEED = 382                            # 478 holes, 6 426 sources


def _balls():
    """the 96^2 room; holes = the covered texels inside eight seeded world-space balls (centres on covered texels, radii 0.4 .. 0.9)"""
    _, pos, nrm, v = ABC.room(96)
    rng = np.random.default_rng(BALL_SEED)
    centres = pos[rng.choice(v, 8, replace=False)].astype(F64)
    radii = rng.uniform(0.4, 0.9, 8)
    d = np.linalg.norm(pos[v].astype(F64)[:, None] - centres[None], axis=-1)
    inside = (d <= radii[None]).any(1)
    return pos, nrm, ABC.morton(v[~inside], 96), ABC.morton(v[inside], 96)


def _lattice():
    """sources on the integer lattice of the plane z = 0.5 (spacing 1/8: dyadic, every difference and square exact), holes at the cell centres (four
    equidistant sources) and at the edge midpoints (two); ids are shuffled so that the lowest id is nowhere special in space"""
    g = 7
    src = [(i * 0.125, j * 0.125) for i in range(g) for j in range(g)]
    hol = [((i + 0.5) * 0.125, (j + 0.5) * 0.125) for i in range(g - 1) for j in range(g - 1)] + [((i + 0.5) * 0.125, j * 0.125) for i in range(g - 1) for j in range(g)]
    xy = np.array(src + hol, F64)
    perm = np.random.default_rng(17).permutation(len(xy))
    pos = np.zeros((len(xy), 3), F32)
    pos[perm, 0], pos[perm, 1], pos[:, 2] = xy[:, 0], xy[:, 1], 0.5
    nrm = np.tile(np.array([0, 0, 1], F32), (len(xy), 1))
    return Case("lattice_tie", pos, nrm, np.sort(perm[:len(src)]), perm[len(src):], 0.5, 1.0)


def _edge():
    """four holes 8 apart, one source each, cos_fill = max_dist = 0.5 (c2 = r2 = 0.25 exactly):
    0: source at distance 0.5: dd == r2 exactly -> within;  1: at nextafter(0.5): dd one ulp above r2 -> out;
    2: nt = (1,1,0), ns = (1,0,1): ns ns = 1 == (0.25 * 2) * 2 exactly -> compatible;  3: ns = (1,0,1 + 2^-20): nn_s larger -> incompatible"""
    up = np.nextafter(F32(0.5), F32(1))
    pos = np.array([(0, 0, 0), (0, 8, 0), (0, 16, 0), (0, 24, 0), (0.5, 0, 0), (up, 8, 0), (0.25, 16, 0), (0.25, 24, 0)], F32)
    nrm = np.array([(0, 0, 1), (0, 0, 1), (1, 1, 0), (1, 1, 0), (0, 0, 1), (0, 0, 1), (1, 0, 1), (1, 0, 1 + 2.0 ** -20)], F32)
    return Case("edge_of_range", pos, nrm, [4, 5, 6, 7], [0, 1, 2, 3], 0.5, 0.5)


def case(name):
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng([41, sum(name.encode())])
    if name == "room64_bake":
        # what the bake's float32 restatement leaves of the 64^2 room under 2 x 2 views
        b = ABC.case("room64")
        view = ABC.bake_f32(b)[0]
        L = b.listed()
        c = Case(name, b.pos, b.nrm, L[view[L] >= 0], L[view[L] < 0])
    elif name == "room64_far":
        c = case("room64_bake").with_(name, max_dist=1.0)
    elif name == "room96_balls":
        pos, nrm, s, h = _balls()
        c = Case(name, pos, nrm, s, h)
    elif name == "lattice_tie":
        c = _lattice()
    elif name == "edge_of_range":
        c = _edge()
    elif name == "no_sources":
        b = case("room64_bake")
        c = b.with_(name, sources=np.zeros(0, np.int32), holes=b.holes[:100])
    elif name == "all_incompatible":
        # holes and sources interleaved on one plane, the sources facing the other way
        xy = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.0625
        pos = np.concatenate([xy, np.full((len(xy), 1), 0.25)], 1)
        ids = np.arange(len(xy))
        nrm = np.where((ids % 2 == 0)[:, None], np.array([[0, 0, 1.0]]), np.array([[0, 0, -1.0]]))
        c = Case(name, pos, nrm, ids[ids % 2 == 1], ids[ids % 2 == 0], 0.5, 0.5)
    elif name in ("raw_normals", "raw_normals_unit"):
        # the balls with 5 % of the normals zeroed; `raw_normals` also scales every normal to a length of 0.3 .. 3
        b = case("room96_balls")
        r = np.random.default_rng(43)
        nrm = b.nrm.copy()
        nrm[r.random(b.Nt) < 0.05] = 0
        if name == "raw_normals":
            nrm = nrm * r.uniform(0.3, 3.0, (b.Nt, 1)).astype(F32)
        c = b.with_(name, nrm=nrm)
    elif name.startswith("list_"):
        # list_h<n_holes>_s<n_src>: the 96^2 room, random sources, Morton-ordered holes from the rest
        nh, ns = int(name.split("_")[1][1:]), int(name.split("_")[2][1:])
        _, pos, nrm, v = ABC.room(96)
        pick = rng.permutation(v)
        c = Case(name, pos, nrm, pick[:ns], ABC.morton(np.sort(pick[ns:ns + nh]), 96), 0.5, 1.5)
    elif name == "shuffled_holes":
        # consecutive holes are no neighbours: every wave's box spans the whole room
        b = case("room96_balls")
        c = b.with_(name, holes=np.random.default_rng(44).permutation(b.holes))
    elif name == "dup_oor":
        b = case("room64_bake")
        junk = np.array([-3, b.Nt, b.Nt + 17, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
        s = np.concatenate([b.sources[:400], junk, b.sources[100:300], b.holes[5:9]])     # four texels are in both lists
        h = np.concatenate([junk[:2], b.holes[:150], b.holes[20:90], junk[2:]])
        c = b.with_(name, sources=s, holes=h, bounds=b.bounds)
    elif name == "inf_dist":
        c = case("room64_bake").with_(name, max_dist=np.inf)
    elif name == "bounds_exclude":
        # the box stops at the 2/3 quantile of x: a third of the positions lie outside it
        b = case("room96_balls")
        ids = np.concatenate([b.valid_sources(), b.valid_holes()])
        bd = b.bounds.copy()
        bd[3] = np.quantile(b.pos[ids, 0], 2.0 / 3.0)
        c = b.with_(name, bounds=bd)
    else:
        raise KeyError(name)
    _CACHE[name] = c
    return c


LISTS = tuple("list_h%d_s%d" % (h, s) for h in LIST_HOLES for s in LIST_SOURCES)
ALL = ("room64_bake", "room64_far", "room96_balls", "lattice_tie", "edge_of_range", "no_sources", "all_incompatible", "raw_normals", "raw_normals_unit",
       "shuffled_holes", "dup_oor", "inf_dist", "bounds_exclude") + LISTS
# where each mutant must be rejected
MUTANT_CASES = {"no_normal": "room64_bake", "no_range": "room64_bake", "farthest": "room64_bake", "tie_high": "lattice_tie", "manhattan": "room96_balls",
                "unit_normals": "raw_normals", "holes_as_sources": "room64_bake"}
