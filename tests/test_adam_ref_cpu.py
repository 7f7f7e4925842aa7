"""Proves the checker of tests/adam_cases.py without a GPU: the op-by-op float32 emulation of the optimiser kernels passes every case of the matrix
through the same check functions the GPU module uses, the legitimate two-rounding form of the first moment passes, every operator mutant is rejected in
every family and form with a non-zero gradient, the adam_tick reference reproduces hand values, and every case satisfies the bound's conditions
(e(den) < den/2, finite reference: asserted inside adam_cases.reference)."""
import numpy as np
import pytest

import adam_cases as AC


def _all_tex_cases():
    for group in AC.TEX_GROUPS:
        for spec in AC.tex_specs(group):
            yield AC.tex_case(*spec)
    for name in AC.BATCHES:
        for variant in (0, 1):
            yield from AC.batch_cases(name, variant)


def test_emulation_passes_every_flat_case():
    worst = 0.0
    for spec in AC.flat_specs():
        c = AC.flat_case(*spec)
        for extra in (0, 1):
            rs = AC.check_outputs(AC.reference(c, extra_u=extra), AC.emulate(c), what=str(spec[:2]))
            worst = max([worst] + list(rs.values()))
    print("worst error / e of the float32 chain, flat kernel: %.3f" % worst)


@pytest.mark.parametrize("group", AC.TEX_GROUPS + ("batch",))
def test_emulation_passes_every_texture_case(group):
    if group == "batch":
        cases = [c for name in AC.BATCHES for variant in (0, 1) for c in AC.batch_cases(name, variant)]
    else:
        cases = [AC.tex_case(*s) for s in AC.tex_specs(group)]
    assert cases
    worst = 0.0
    for c in cases:
        ref = AC.reference(c)
        rs = AC.check_outputs(ref, AC.emulate(c), what=str((c.H, c.W, c.C) + c.form))
        assert (ref["mip1"] is not None) == c.mip
        worst = max([worst] + list(rs.values()))
    print("worst error / e of the float32 chain, %s: %.3f" % (group, worst))


def _mutant_cases():
    """flat and texture forms x the families with a non-zero gradient, clamp (1e-2, 0.8) so that a missing clamp shows; steps and eps rotate (the flat
    kernel and one texture form take all of them)"""
    out = []
    seed = 50000
    for fam in AC.NONZERO:
        for eps in AC.EPSS:
            for step in AC.STEPS:
                s = (fam, AC.CLAMPS[0], eps, step)
                seed += 1
                out.append(AC.flat_case(257, s, seed))
                out.append(AC.tex_case("mut", 8, 644, 3, "masked", True, True, True, s, seed, "half", mask1="half"))
        i = 0
        for (H, W, C) in ((4, 324, 3), (8, 644, 3), (4, 342, 3)):
            for (g0mode, g1, g2, mip) in AC.pointer_combos(H, W):
                for m1 in ((None, "half") if (g1 and g2) else (None,)):
                    i += 1
                    seed += 1
                    s = (fam, AC.CLAMPS[0], AC.EPSS[i % 2], AC.STEPS[i % 3])
                    out.append(AC.tex_case("mut", H, W, C, g0mode, g1, g2, mip, s, seed, "half", mask1=m1))
    return out


def test_legitimate_two_rounding_first_moment_passes():
    worst = 0.0
    for c in _mutant_cases():
        rs = AC.check_outputs(AC.reference(c), AC.emulate(c, "two_rounding_m"))
        worst = max([worst] + list(rs.values()))
    print("worst error / e of m * b1 + g * (1 - b1): %.3f" % worst)


@pytest.mark.parametrize("mut", AC.MUTANTS)
def test_mutant_is_rejected_in_every_family_and_form(mut):
    seen = set()
    for c in _mutant_cases():
        if not AC.mutant_applies(mut, c):
            continue
        ref = AC.reference(c, extra_u=1)                               # (the wider of the two bounds)
        assert AC.accepts(ref, AC.emulate(c)), "the unmutated chain must pass"
        rs = AC.ratios(ref, AC.emulate(c, mut))
        assert not AC.accepts(ref, AC.emulate(c, mut)), "mutant %s passes: family %s form %s ratios %s" % (mut, c.family, c.form, rs)
        seen.add((c.family, c.form[0]))
    fams = {f for f, _ in seen}
    assert fams == set(AC.NONZERO), fams
    if mut in ("omb2_decimal", "eps_in_root", "no_bias", "no_clamp"):
        assert {g for _, g in seen} == {"flat", "mut"}


def test_zero_gradient_cannot_see_gradient_mutants_and_other_families_cover_every_form():
    s = ("zerograd", AC.CLAMPS[0], AC.EPSS[0], 3)
    c = AC.tex_case("mut", 8, 644, 3, "masked", True, True, True, s, 1, "half", mask1="half")
    ref = AC.reference(c)
    for mut in ("l2_axis", "fold1_half", "fold0_half"):
        assert AC.accepts(ref, AC.emulate(c, mut))
    # every form of the GPU matrix is run with a non-zero gradient at least once
    forms, covered = set(), set()
    for spec in AC.flat_specs():
        if spec[0] > 0:
            forms.add(("flat", spec[0]))
            if spec[1][0] != "zerograd":
                covered.add(("flat", spec[0]))
    for c in _all_tex_cases():
        key = (c.H, c.W, c.C) + c.form
        forms.add(key)
        if c.family != "zerograd":
            assert np.abs(AC.folded_gradient(c)[0]).max() > 0
            covered.add(key)
    assert forms == covered, sorted(forms - covered)
    # and the matrix holds every family, clamp, eps and step in the flat and in the texture form, every mask pattern, every pointer combination
    assert {s[1] for s in AC.flat_specs()} == set(AC.SETTINGS)
    assert {s[8] for s in AC.tex_specs("settings")} == set(AC.SETTINGS)
    assert {s[10] for s in AC.tex_specs("patterns")} == set(AC.MASK_PATTERNS)
    for (H, W, C) in AC.CROSS_SHAPES:
        assert {s[4:8] for s in AC.tex_specs("cross") if s[1:4] == (H, W, C)} == set(AC.pointer_combos(H, W))
    for group in ("vector", "scalar", "forced_scalar", "grid_y"):
        for shape in {s[1:4] for s in AC.tex_specs(group)}:
            mine = [s for s in AC.tex_specs(group) if s[1:4] == shape]
            assert {s[4] for s in mine} == {"dense", "masked", "null"} and {s[7] for s in mine} == {True, False}
            if shape[0] % 4 == 0 and shape[1] % 4 == 0:
                assert {s[5] for s in mine} == {True, False} and {s[6] for s in mine} == {True, False}


def test_matrix_shapes_take_the_paths_they_are_meant_for():
    epb = lambda C: 960 if C == 3 else 1024
    for (H, W, C) in AC.VEC_SHAPES + (AC.GRID_Y_SHAPE,) + AC.FORCED_SCALAR_SHAPES:
        assert (W * C) % 4 == 0 and H % 2 == 0 and W % 2 == 0
    for (H, W, C) in AC.SCALAR_SHAPES:
        assert (W * C) % 4 != 0 and (H % 4 or W % 4)
    segs = {s: -(-s[1] * s[2] // epb(s[2])) for s in AC.VEC_SHAPES}
    assert segs[(6, 320, 3)] == 1 and 320 * 3 == 960 and segs[(4, 324, 3)] == 2 and segs[(8, 644, 3)] == 3
    assert segs[(4, 1028, 1)] == 2 and segs[(4, 516, 2)] == 2 and segs[(4, 260, 4)] == 2
    assert 4100 // 2 > 2048 and 8196 // 2 > 4096 and -(-(342 // 2) * 3 // 256) == 3 and (342 // 2) * 3 - 512 == 1
    assert -(-(AC.GRID_Y_SHAPE[0] // 2) // AC.GRID_Y) == 4 and (AC.GRID_Y_SHAPE[0] // 2) % AC.GRID_Y != 0
    assert max(AC.FLAT_N) > 4096 * 256
    for name, jobs in AC.BATCHES.items():
        assert 1 <= len(jobs) <= 4
    assert {len(j) for j in AC.BATCHES.values()} == {1, 2, 3, 4}
    assert {frozenset(j[2] for j in jobs) for jobs in AC.BATCHES.values()} >= {frozenset({1}), frozenset({3}), frozenset({1, 3}), frozenset({1, 2, 3, 4})}


def test_mask_layout():
    bits = np.zeros(70, bool)
    bits[[0, 31, 32, 69]] = True
    w = AC.pack_mask(bits)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]
    assert (AC.unpack_mask(w, 70) == bits).all()
    for pat in AC.MASK_PATTERNS:
        b = AC.mask_bits(pat, 1296, np.random.default_rng(0))
        assert b.sum() == {"none": 0, "all": 1296}.get(pat, b.sum()) and (pat in ("none", "all", "half") or b.sum() == 1)
    assert AC.mask_bits("last", 1296, None)[1295] and AC.mask_bits("bit32", 1296, None)[32]


def test_tick_reference_hand_values():
    import mpmath
    lr = 3e-2
    s, ss, bc = AC.tick_exact(0.0, lr, 0.9, 0.999)
    assert s == 1.0
    with mpmath.workprec(200):
        assert abs(ss - mpmath.mpf(lr) / (1 - mpmath.mpf(0.9))) < mpmath.mpf(10) ** -55
        assert abs(bc - mpmath.sqrt(1 - mpmath.mpf(0.999))) < mpmath.mpf(10) ** -55
    assert abs(float(ss) - lr / 0.1) < 1e-15 and abs(float(bc) - 0.001 ** 0.5) < 1e-15           # lr / 0.1 and sqrt(0.001) up to the betas' own rounding
    s, ss, bc = AC.tick_exact(9.0, lr, 0.0, 0.0)
    assert s == 10.0 and float(ss) == lr and float(bc) == 1.0
    s, ss, bc = AC.tick_exact(1e7 - 1, lr, 0.9, 0.999)
    assert s == 1e7 and float(ss) == lr and float(bc) == 1.0
    assert AC._f32_round(ss) == np.float32(lr)
    lo, mid, hi = AC.tick_allowed(mpmath.mpf(1))
    assert mid == 1 and lo == np.float32(1 - 2.0 ** -24) and hi == np.float32(1 + 2.0 ** -23)


def test_tick_checker_accepts_float64_evaluation_and_rejects_wrong_records():
    for n in AC.TICK_N:
        st, hy = AC.tick_state(n, 0)
        for mask in AC.tick_masks(n):
            st1, hy1 = st.copy(), hy.copy()
            for i in range(n):
                if (mask >> i) & 1:
                    st1[i, 0] += 1
                    hy1[i] = (st[i, 1] / (1.0 - st[i, 2] ** st1[i, 0]), np.sqrt(1.0 - st[i, 3] ** st1[i, 0]))
            AC.check_tick(st, hy, mask, st1, hy1)
            if mask:
                i = mask.bit_length() - 1
                bad = hy1.copy()
                bad[i, 0] = np.nextafter(np.nextafter(bad[i, 0], np.float32(9)), np.float32(9)) * np.float32(1 + 2.0 ** -20)
                with pytest.raises(AssertionError):
                    AC.check_tick(st, hy, mask, st1, bad)
                with pytest.raises(AssertionError):                       # a record shifted by one: the neighbour's pair
                    AC.check_tick(st, hy, mask, st1, np.roll(hy1, 1, axis=0) if n > 1 else hy)
            if mask != ((1 << n) - 1 if n else 0):
                i = [k for k in range(n) if not (mask >> k) & 1][0]
                bad = st1.copy()
                bad[i, 0] += 1
                with pytest.raises(AssertionError):
                    AC.check_tick(st, hy, mask, bad, hy1)


def test_grad_add_checker():
    for fam in AC.FAMILIES:
        for pat in AC.MASK_PATTERNS:
            c = AC.grad_add_case(70, 3, pat, fam, 7)
            on = np.broadcast_to(c.bits[:, None], c.g.shape)
            got = np.where(on, c.g + np.where(on, c.g0, np.float32(0)), c.g).astype(np.float32)
            AC.check_grad_add(c, got)
            if fam != "zerograd" and c.bits.any() and not c.bits.all():
                with pytest.raises(AssertionError):
                    AC.check_grad_add(c, np.where(np.roll(on, 1, axis=0), c.g + np.nan_to_num(c.g0), c.g).astype(np.float32))
            plus = c.g + np.float32(0)                                    # -0 + 0 = +0: changed bits where the mask is clear
            if not c.bits.all():
                with pytest.raises(AssertionError):
                    AC.check_grad_add(c, np.where(on, got, plus).astype(np.float32))
