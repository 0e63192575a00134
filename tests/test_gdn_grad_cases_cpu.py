"""tests/gdn_grad_cases.py without a GPU: the formulas against float64 autograd of the composition, the exact tier's domain, the case list against the
restated geometry, and every broken-kernel model detected."""
import numpy as np
import pytest
import torch

import gdn_grad_cases as gc

IDS = [c.name for c in gc.CASES]


@pytest.mark.parametrize("case", [c for c in gc.CASES if c.c <= 64 or c.name.startswith("b192_p777")], ids=lambda c: c.name)
@pytest.mark.parametrize("tier", ["exact", "integer"])
def test_formulas_match_float64_autograd(case, tier):
    data = gc.make_exact(case) if tier == "exact" else gc.make_integer(case)
    x = torch.from_numpy(data["x"]).double().requires_grad_(True)
    gamma = torch.from_numpy(data["gamma"]).double().requires_grad_(True)
    beta = torch.from_numpy(data["beta"]).double().requires_grad_(True)
    gc.composition(x, gamma, beta, case.inverse).backward(torch.from_numpy(data["gy"]).double())
    ref = gc.reference(case, data, np.float64)
    for name, got in (("gx", x.grad), ("ggamma", gamma.grad), ("gbeta", beta.grad)):
        got, want = got.numpy(), ref[name]
        scale = max(float(np.abs(got).max()), 1e-300)
        assert float(np.abs(got - want).max()) <= 1e-12 * scale, (case.name, tier, name, float(np.abs(got - want).max()), scale)


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_exact_tier_is_exact_in_fp32(case):
    data = gc.make_exact(case)
    m = gc.assert_exact_domain(case, data)
    want = gc.as_fp32(gc.reference(case, data, np.float32))                 # every expected value is an fp32 number ...
    ref64 = gc.reference(case, data, np.float64)
    for k in want:                                                          # ... and the fp32 evaluation equals the float64 one
        assert np.array_equal(want[k].astype(np.float64), ref64[k]), (case.name, k)
    assert 1 <= m <= 7 and np.any(want["gx"] != 0) and np.any(want["ggamma"] != 0) and np.any(want["gbeta"] != 0)


def test_exact_domain_refuses_what_lies_outside():
    case = gc.CASES[0]
    data = gc.make_exact(case)
    with pytest.raises(AssertionError):
        gc.assert_exact_domain(case, dict(data, beta=data["beta"] + 1))
    with pytest.raises(AssertionError):
        gc.assert_exact_domain(case._replace(n=3, h=100, w=100), data)


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_integer_tier_restatement_and_bounds(case):
    data = gc.make_integer(case)
    t32, t64 = gc.reference(case, data, np.float32)["t"], gc.reference(case, data, np.float64)["t"]
    assert float(np.abs(t32 - t64).max()) <= 4 * gc.EPS * float(np.abs(t64).max()) and np.any(t32 != t64)      # real norms: the t-map does round
    b = gc.integer_bounds(case, data)
    ref = gc.reference(case, data, np.float64)
    for k in ("gx", "ggamma", "gbeta"):                                     # a bound, not a licence: far below the values it guards
        assert b[k].shape == ref[k].shape and np.all(b[k] >= 0)
        assert float(b[k].max()) < 1e-3 * float(np.abs(ref[k]).max()), (case.name, k)


def test_case_list_reaches_every_class():
    geos = {c.name: gc.geometry(c) for c in gc.CASES}
    assert {c.c for c in gc.CASES} == set(gc.CHANNELS)
    assert {35, 64, 65, 66, 128, 777} <= {c.h * c.w for c in gc.CASES}
    assert {c.n for c in gc.CASES} == {1, 3} and {c.inverse for c in gc.CASES} == {False, True}
    for ch in gc.CHANNELS:                                                  # both access forms of every channel count's kernels would be 14 more cases;
        assert any(c.c == ch for c in gc.CASES)                             # every count has one, 16 .. 192 have both between them:
    assert {(c.c, geos[c.name].vec) for c in gc.CASES} >= {(16, True), (16, False), (192, True), (192, False), (64, False), (96, True), (96, False)}
    assert any(c.misaligned and (c.h * c.w) % 4 == 0 for c in gc.CASES)
    assert any(g.ntiles == 1 and g.nsplit == 1 for g in geos.values())                                        # one split
    several = [g for g in geos.values() if g.tps > 1 and g.ntiles % g.tps]
    assert several and all(g.nsplit > 1 and g.ntiles > gc.MAX_SPLITS for g in several)                        # several splits, a short last one, more tiles than splits
    assert any(c.n > 1 and (c.h * c.w) % gc.TILE for c in gc.CASES)                                           # a tile that ends an image
    assert any(c.n > 1 and c.inverse for c in gc.CASES) and any(c.c == 192 and c.inverse for c in gc.CASES)
    m = gc.geometry(gc.MODULE_CASE)
    assert (gc.MODULE_CASE.c, gc.MODULE_CASE.h, gc.MODULE_CASE.w, gc.MODULE_CASE.n) == (192, 68, 132, 1) and m.tps == 2 and m.nsplit == 141
    for c in gc.CASES + [gc.MODULE_CASE]:                                   # small: a few seconds each on the GPU, the references in seconds here
        assert c.n * c.c * c.h * c.w <= 192 * 68 * 132


def test_geometry_is_monotone_where_the_scratch_must_be():
    prev = 0
    for p in (1, 31, 32, 33, 64, 8160, 8192, 8193, 16384, 16416, 100000):
        cur = gc.geometry(gc.GradCase("g", 192, 1, 1, p, False, False)).scratch_bytes
        assert cur > prev
        prev = cur
    g512, g513 = (gc.geometry(gc.GradCase("g", 16, 1, 1, 32 * k, False, False)) for k in (512, 513))
    assert (g512.nsplit, g513.nsplit) == (256, 171)                         # the split count itself can shrink; the scratch is sized by its bound


@pytest.mark.parametrize("mut", sorted(gc.MUTATIONS))
def test_every_broken_kernel_model_is_detected(mut):
    hit = {}
    for tier, make in (("exact", gc.make_exact), ("integer", gc.make_integer)):
        for case in gc.CASES:
            if case.c > 64 and not case.name.startswith("b192_p777"):      # (the references of the wide cases cost seconds and add no class)
                continue
            if gc.MUTATIONS[mut](case):
                ch = gc.changed(case, make(case), mut)
                assert ch, (mut, tier, case.name)                           # wherever the model applies, some output changes
                hit.setdefault(tier, set()).update(ch)
    assert set(hit) == {"exact", "integer"}, (mut, hit)
    expected = {"gamma_not_transposed": {"gx"}, "direction_ignored": {"t", "gx", "ggamma", "gbeta"}, "half_missing": {"ggamma", "gbeta"},
                "t_over_n": {"t", "gx", "ggamma", "gbeta"}, "x_not_squared": {"ggamma"}, "last_tile_dropped": {"ggamma", "gbeta"},
                "last_split_dropped": {"ggamma", "gbeta"}, "split_twice": {"ggamma", "gbeta"}, "first_image_only": {"ggamma"}, "beta_rotated": {"gbeta"}}[mut]
    for tier in hit:
        assert hit[tier] == expected, (mut, tier, hit[tier])
