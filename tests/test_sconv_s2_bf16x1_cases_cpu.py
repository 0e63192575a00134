"""tests/sconv_s2_bf16x1_cases.py checked by itself, without a GPU: the case list reaches all four k_sconv_b1s2 bodies and, for both kernel sizes, the
chunk counts 1, even and odd above 1 (the bodies alternate their ring sets by chunk parity); the exactness condition holds for every case and tier on
the rounded operands; every rounding tier of every case holds values that round up, round down and tie to both sides; and each applicable mutation --
the arithmetic ones of tests/sconv_bf16x1_cases.py, the geometry ones of tests/sconv_s2_cases.py -- changes the reference of a case it applies to."""
import numpy as np
import pytest

import sconv_s2_bf16x1_cases as sb
import sconv_s2_cases as s2

MUTATION_MACS = 4e9                                                        # as tests/test_sconv_s2_cases_cpu.py: the production cases above it differ in map size only


def _macs(c):
    return float(c.n) * c.cin * c.cout * c.ks * c.ks * c.hp * c.wp


MUTATED = [c for c in sb.CASES if _macs(c) <= MUTATION_MACS]


def test_the_case_list_is_the_32_channel_part_of_the_stride_2_list_plus_odd_chunk_counts():
    assert [c for c in sb.CASES if c not in sb.ODD_CHUNKS] == [c for c in s2.CASES if c.cin % 32 == 0]
    assert all(sb.supported(c.cin, c.cout, c.ks) for c in sb.CASES) and len({c.name for c in sb.CASES}) == len(sb.CASES)
    assert not sb.supported(16, 192, 3) and not sb.supported(48, 192, 1) and sb.supported(32, 96, 3) and not sb.supported(32, 100, 1)
    assert [c.name for c in sb.PRODUCTION] == [c.name for c in s2.PRODUCTION]                       # all five production shapes are 192 -> 192
    br = [(c, sb.branch_of(c)) for c in sb.CASES]
    assert {(b.nq, b.rw, b.ks) for c, b in br} == sb.BODIES
    have = lambda p: any(p(c, b) for c, b in br)
    for ks in (3, 1):
        for what, p in (("one chunk", lambda c, b: b.chunks == 1), ("an even chunk count", lambda c, b: b.chunks % 2 == 0),
                        ("an odd chunk count above 1", lambda c, b: b.chunks % 2 == 1 and b.chunks > 1), ("six chunks", lambda c, b: b.chunks == 6),
                        ("n = 3", lambda c, b: c.n == 3), ("ragged rows", lambda c, b: b.rem != 0), ("ragged columns", lambda c, b: s2.out_hw(c)[1] % 16 != 0),
                        ("blockIdx.y 0 .. 1", lambda c, b: b.blocks_y == 2), ("pad 3", lambda c, b: c.pad == 3), ("a residual", lambda c, b: c.res),
                        ("no slope", lambda c, b: not c.slope), ("one tile of 32 channels", lambda c, b: c.cin == 32 and b.tiles_y * b.tiles_x * c.n == 1)):
            assert have(lambda c, b, p=p, ks=ks: b.ks == ks and p(c, b)), (ks, what)
    for oring in (0, 1, 2):
        assert have(lambda c, b: c.oring == oring), oring
    assert have(lambda c, b: c.ks == 3 and c.sphere == 1 and c.pad == 3) and have(lambda c, b: c.ks == 3 and c.sphere == 0)
    for nq in (4, 2):                                                       # the parity alternation in each 3x3 and 1x1 body
        for ks in (3, 1):
            assert have(lambda c, b: (b.nq, b.ks) == (nq, ks) and b.chunks % 2 == 1 and b.chunks > 1), (nq, ks)


@pytest.mark.parametrize("tier", list(sb.TIERS))
def test_exact_domain_and_rounding_classes_of_every_case(tier):
    """|b| + 4 |res| + sum |w~||x~| < 2^24 for every case (the large production cases through their ranges: rounding moves a magnitude up by at most 2^-8
    of itself), and the tier's own operand holds every rounding class while the other needs no rounding"""
    xm, wm = sb.TIERS[tier]
    ran = 0
    for c in sb.CASES:
        assert (1 + 2.0 ** -8) ** 2 * c.cin * c.ks * c.ks * xm * wm + 5 * sb.EPILOGUE_MAX < float(1 << 24), c.name
        if _macs(c) > MUTATION_MACS:
            continue
        data = sb.make_case(c, tier)
        bound = sb.assert_exact_domain(c, data)
        assert float(np.abs(data["x"]).max()) <= xm and float(np.abs(data["w"]).max()) <= wm and 0 < bound < float(1 << 24)
        interior = data["x"][:, :, c.pad:c.hp - c.pad, c.pad:c.wp - c.pad]
        cx, cw = sb.rounding_classes(interior), sb.rounding_classes(data["w"])
        allc = {"exact", "down", "up", "tie_down", "tie_up"}
        assert cx == (allc if tier == "xrnd" else {"exact"}), (c.name, tier, cx)
        assert cw == (allc if tier == "wrnd" else {"exact"}), (c.name, tier, cw)
        assert (sb.bf16_rne(data["b"]) != data["b"]).mean() > 0.25, c.name                            # most biases are not bf16 numbers
        assert data["res"] is None or (sb.bf16_rne(data["res"]) != data["res"]).mean() > 0.25
        ran += 1
    assert ran >= len(sb.SMALL)


@pytest.mark.parametrize("case,tier", [(c, t) for c in MUTATED for t in sb.TIERS], ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_mutation_changes_the_reference(case, tier):
    data = sb.make_case(case, tier)
    want = sb.reference(case, data)
    assert want.shape == sb.out_shape(case) and np.array_equal(want, want.astype(np.float32).astype(np.float64))       # the expected values are fp32 numbers
    frame = want == sb.SENTINEL
    assert frame.mean() < 1 and (frame.any() or case.oring == 0)
    muts = [m for m, applies in sb.MUTATIONS_ARITHMETIC.items() if applies(case, tier)]
    if tier == "hi":                                                        # the geometry mutations run on the hi tier's data
        muts += [m for m, applies in sb.MUTATIONS_GEOMETRY.items() if applies(case)]
    assert muts
    for m in muts:
        got = sb.reference(case, data, m)
        assert got.shape == want.shape and not np.array_equal(got, want), "%s / %s: mutation %s is invisible" % (case.name, tier, m)
    if tier == "hi":                                                        # nothing rounds: the form's result is the exact convolution
        assert np.array_equal(want, s2.reference(case, data)) and np.array_equal(want, sb.reference(case, data, "truncation"))
    else:                                                                   # rounding changes a large share of the outputs, not a few
        assert (sb.reference(case, data, "lo_added") != want)[~frame].mean() > 0.25


def test_every_mutation_applies_somewhere():
    """no applicable mutation is left unexercised: each applies to a case the test above runs, on the tier meant to catch it"""
    for m, applies in sb.MUTATIONS_ARITHMETIC.items():
        assert any(applies(c, t) for c in MUTATED for t in sb.TIERS), m
    for m, applies in sb.MUTATIONS_GEOMETRY.items():
        assert any(applies(c) for c in MUTATED), m
    assert set(sb.MUTATIONS_ARITHMETIC) == {"truncation", "half_away", "x_not_rounded", "w_not_rounded", "lo_added", "bias_rounded", "res_rounded"}
    assert {"taps_on_2i_plus_1", "stride_rows_only", "stride_cols_only", "stride_1_read", "res_on_input_grid", "chunk_twice", "prev_image"} <= set(sb.MUTATIONS_GEOMETRY)
