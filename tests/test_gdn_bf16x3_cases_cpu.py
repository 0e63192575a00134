"""tests/gdn_bf16x3_cases.py checked by itself, without a GPU: the case list reaches every k_gdn_b3<C, VEC> and every position-tile situation, the integer
data is in the exact domain and holds every rounding class, each bug a kernel could have changes the reference, and on the real-valued data of the parity
test the 2^-15 bound passes the split form's arithmetic and fails a form without lo parts."""
import numpy as np
import pytest

import gdn_bf16x3_cases as gc


def test_case_list_covers_the_kernels():
    """which instantiation each case reaches, and that all ten are reached; P below a tile, one tile, one tile + 1, odd, P % 4 == 2, several tiles; n = 3; a
    misaligned view; both directions for every channel count; the six production maps at n = 1"""
    reached = {}
    for c in gc.SMALL:
        reached.setdefault(gc.branch_of(c), []).append(c.name)
    assert set(reached) == gc.INSTANTIATIONS, sorted(gc.INSTANTIATIONS - set(reached))
    ps = [c.h * c.w for c in gc.SMALL]
    assert any(p < gc.PT for p in ps) and gc.PT in ps and gc.PT + 1 in ps and any(p % 2 for p in ps) and any(p % 4 == 2 for p in ps)
    assert any(p >= 4 * gc.PT and p % gc.PT == 0 for p in ps) and any(p > 4 * gc.PT and p % gc.PT for p in ps)
    assert any(c.n == 3 for c in gc.SMALL) and any(c.misaligned and c.h * c.w % 4 == 0 for c in gc.SMALL)
    for ch in gc.CHANNELS:
        assert {c.inverse for c in gc.SMALL if c.c == ch} == {False, True}, ch
    assert len(gc.PRODUCTION) == 6 and all(c.n == 1 and c.c == 192 and gc.branch_of(c) == (192, True) for c in gc.PRODUCTION)
    assert sorted((c.h, c.w, c.inverse) for c in gc.PRODUCTION) == sorted((h, w, inv) for (h, w) in gc._MAPS[:3] for inv in (False, True))
    assert len({c.name for c in gc.CASES}) == len(gc.CASES)


def test_wave_split_tiles_the_channels():
    for c in gc.CHANNELS:
        ncg, npg, mt, ntp = gc.wave_split(c)
        assert ncg * npg == 4 and ncg * mt * 16 == c and npg * ntp * 16 == gc.PT
    assert [gc.supported(c) for c in (16, 32, 48, 64, 96, 100, 128, 192, 224)] == [False, True, False, True, True, False, True, True, False]


def test_packed_layout_holds_every_part_once():
    c = 96
    gamma = (np.arange(c * c, dtype=np.float32).reshape(c, c) + 0.5) * 3.0      # distinct values with lo parts
    flat = gc.packed_layout(gamma)
    hi, lo = gc.split(gamma)
    assert flat.size == 2 * c * c
    cells = flat.reshape(-1, 2, 64, 8)                                      # [(cg, s, m)][hl][lane][j]
    assert sorted(cells[:, 0].ravel().tolist()) == sorted(hi.ravel().tolist()) and sorted(cells[:, 1].ravel().tolist()) == sorted(lo.ravel().tolist())
    ncg, _, mt, _ = gc.wave_split(c)
    cg, s, m, lane, j = 1, 2, 1, 37, 5
    assert cells[(cg * (c // 32) + s) * mt + m, 1, lane, j] == lo[16 * (cg * mt + m) + lane % 16, 32 * s + 8 * (lane // 16) + j]


SMALL_BY_TIER = [(c, t) for c in gc.SMALL for t in gc.TIERS]


@pytest.mark.parametrize("case,tier", [(c, t) for c in gc.CASES for t in gc.TIERS], ids=lambda v: getattr(v, "name", v))
def test_exact_domain(case, tier):
    if case.prod and case.h * case.w > 132 * 260:
        data = gc.make(case._replace(h=8, w=case.w), tier)                  # the same distribution; the bound takes maxima over cells
    else:
        data = gc.make(case, tier)
    assert gc.assert_exact_domain(case, data) < gc.EXACT_BELOW


@pytest.mark.parametrize("case,tier", SMALL_BY_TIER, ids=lambda v: getattr(v, "name", v))
def test_data_holds_what_the_tier_is_for(case, tier):
    data = gc.make(case, tier)
    sq = (data["x"] * data["x"]).astype(np.float32)
    glo, slo = gc.split(data["gamma"])[1], gc.split(sq)[1]
    if tier == "hi":
        assert not glo.any() and not slo.any()
        assert gc.perfect_squares(data).any()
        return
    assert slo.any() and glo.any() == (tier == "both")
    for part in gc.split(sq) + gc.split(data["gamma"]):
        assert np.array_equal(part, np.rint(part))
    cls = gc.rounding_classes(sq) | gc.rounding_classes(data["gamma"])
    # values that round up, round down and tie: squares tie down only (gdn_bf16x3_cases' docstring), the `both` tier's large gammas are ties to both sides
    assert ({"up", "down", "tie_down"} if tier == "xsq" else {"tie_up", "tie_down"}) <= cls, cls
    if tier == "both":                                                      # the reference differs from the plain sum by exactly the dropped lo lo terms
        plain = np.matmul(data["gamma"].astype(np.float64)[None], sq.astype(np.float64).reshape(sq.shape[0], case.c, -1)) + data["beta"].astype(np.float64)[None, :, None]
        assert np.array_equal(gc.sums(data, "lo_lo_added").reshape(plain.shape), plain) and not np.array_equal(gc.sums(data).reshape(plain.shape), plain)


@pytest.mark.parametrize("case,tier", SMALL_BY_TIER, ids=lambda v: getattr(v, "name", v))
def test_every_mutation_changes_the_reference(case, tier):
    data = gc.make(case, tier)
    want = gc.reference(case, data)
    assert np.isfinite(want).all()
    applied = 0
    for mut, applies in gc.MUTATIONS.items():
        if applies(case, tier):
            applied += 1
            assert not np.array_equal(gc.reference(case, data, mut), want, equal_nan=True), mut
    assert applied >= 5
    assert set(gc.MUTATIONS) >= set(gc.GDN_MUTATIONS) | {"lo_dropped", "lo_lo_added", "truncation", "beta_rounded"}


def test_every_mutation_applies_somewhere():
    for mut, applies in gc.MUTATIONS.items():
        assert any(applies(c, t) for c, t in SMALL_BY_TIER), mut


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0])
@pytest.mark.parametrize("c", [96, 192])
def test_the_bound_tells_the_split_form_from_a_form_without_lo(c, scale, inverse):
    """on the parity test's data: the split form's operand arithmetic sits well inside 2^-15, hi parts alone break it, and so does rounding x before squaring"""
    gamma, beta = gc.effective(*gc.real_params(c, 0))
    assert gamma.min() >= 0 and beta.min() > 0
    x = gc.real_x(c, scale)
    want = gc.gdn_float64(x, gamma, beta, inverse)
    assert gc.max_rel_err(gc.emulate(x, gamma, beta, inverse), want) < gc.BOUND / 2
    assert gc.max_rel_err(gc.emulate(x, gamma, beta, inverse, "hi_only"), want) > gc.BOUND
    assert gc.max_rel_err(gc.emulate(x, gamma, beta, inverse, "x_rounded"), want) > gc.BOUND
