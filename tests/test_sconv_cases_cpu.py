"""tests/sconv_cases.py checked by itself, without a GPU: the case lists reach every branch of sconv_launch / sconv_workgroup / lic360_gdn that
the exact GPU tests claim to reach (asserted, so that a later edit of the lists cannot lose one silently); the exactness condition holds for every
case and tier with the ranges as committed; and the references can tell a wrong kernel from a right one -- each of a list of plausible kernel bugs,
applied to the reference, changes the result on every case it applies to."""
import numpy as np
import pytest
import torch

import sconv_cases as sc

# the mutation and cross-check tests convolve on the CPU in float64: every small case, and the production cases up to this many MACs per
# reference (68 x 132 at 192 -> 192: 2.9e9; a 516 x 1028 reference is 5 s, times 16 mutations).  The production cases above it differ from
# ones below it in their map size only.
MUTATION_MACS = 4e9


def _macs(c):
    return float(c.n) * c.cin * c.cout * c.ks * c.ks * c.hp * c.wp


MUTATED = [c for c in sc.CASES if _macs(c) <= MUTATION_MACS]


def _branches():
    return [(c, sc.branch_of(c, b3)) for c in sc.CASES for b3 in (False, True) if sc.supported(b3, c.cin, c.cout, c.ks)]


def test_every_case_is_a_legal_call():
    """sconv_launch's argument contract, restated: a case the native check would refuse tests nothing"""
    names = [c.name for c in sc.CASES]
    assert len(set(names)) == len(names)
    for c in sc.CASES + [sc.PAST_4GIB]:
        assert sc.forms_of(c), c.name
        assert c.ring >= c.ks // 2 and c.ring_w >= c.ring and c.hp > 2 * c.ring and c.wp > 2 * c.ring_w and 0 <= c.crop <= c.ring, c.name
        assert not c.sphere or (c.ks == 3 and c.pad >= 1 and c.hp >= 4 * c.pad and c.wp >= 4 * c.pad), c.name
        assert not c.res or c.crop == 0 or c.shuffle, c.name
        assert 32.0 * c.hp * c.wp * 4 < 2.0 ** 32, c.name


def test_the_case_list_covers_the_branch_matrix():
    br = _branches()
    have = lambda pred: any(pred(c, b) for c, b in br)
    missing = []
    def need(what, pred):
        if not have(pred):
            missing.append(what)
    for b3 in (False, True):
        for ks in (3, 1):
            f = "%s %dx%d: " % ("bf16x3" if b3 else "fp32", ks, ks)
            mine = lambda p, b3=b3, ks=ks: (lambda c, b: b.b3 == b3 and b.ks == ks and p(c, b))
            for nq in (4, 2):
                q = lambda p, nq=nq, mine=mine: mine(lambda c, b: b.nq == nq and p(c, b))
                need(f + "NQ = %d" % nq, q(lambda c, b: True))
                need(f + "NQ = %d, a window lower than one tile" % nq, q(lambda c, b: b.full == 0))
                need(f + "NQ = %d, three tile rows" % nq, q(lambda c, b: b.tiles_y >= 3))
                if ks == 3:
                    nrg = 8 // nq
                    for rem in range(1, nrg + 1):
                        need(f + "NQ = %d, tall last row with remainder %d" % (nq, rem), q(lambda c, b, rem=rem: b.tall and b.rem == rem and b.rw_last == b.rw + 1))
                    need(f + "NQ = %d, the extra tile row at remainder %d" % (nq, nrg + 1), q(lambda c, b: not b.tall and b.rem == nrg + 1 and b.full >= 1 and b.tiles_y == b.full + 1))
            need(f + "three tile rows, the last one tall", mine(lambda c, b: b.tiles_y >= 3 and b.tall) if ks == 3 else mine(lambda c, b: True))
            need(f + "tile columns exact", mine(lambda c, b: (c.wp - 2 * c.ring_w) % 16 == 0))
            need(f + "tile columns ragged", mine(lambda c, b: (c.wp - 2 * c.ring_w) % 16 != 0))
            need(f + "blockIdx.y up to 3", mine(lambda c, b: b.blocks_y == 4))
            need(f + "one chunk of input channels", mine(lambda c, b: b.chunks == 1))
            need(f + "six chunks of input channels", mine(lambda c, b: b.chunks == 6))
            need(f + "192 input channels", mine(lambda c, b: c.cin == 192))
            for crop in (0, 1):
                need(f + "crop %d" % crop, mine(lambda c, b, crop=crop: c.crop == crop))
            need(f + "crop without shuffle", mine(lambda c, b: c.crop == 1 and not c.shuffle))
            need(f + "shuffle with residual", mine(lambda c, b: c.shuffle and c.res))
            need(f + "shuffle without residual", mine(lambda c, b: c.shuffle and not c.res))
            need(f + "residual without shuffle", mine(lambda c, b: c.res and not c.shuffle))
            need(f + "no slope", mine(lambda c, b: not c.slope))
            need(f + "slope", mine(lambda c, b: c.slope))
            for n in (1, 3):
                need(f + "n = %d" % n, mine(lambda c, b, n=n: c.n == n))
            if ks == 3:
                for sphere in (0, 1, 2):
                    need(f + "sphere %d" % sphere, mine(lambda c, b, sphere=sphere: c.sphere == sphere))
                for pad in (1, 2, 3):
                    need(f + "pad %d under a sphere rule" % pad, mine(lambda c, b, pad=pad: c.sphere != 0 and c.pad == pad))
                need(f + "pole rows read (ring <= pad)", mine(lambda c, b: c.sphere == 1 and c.ring <= c.pad))
                need(f + "ring_w above ring", mine(lambda c, b: c.ring_w > c.ring))
            need(f + "a production shape", mine(lambda c, b: c.prod))
    assert not missing, "the case list lost: " + "; ".join(missing)
    # every body instantiation: (NQ, RW of the body, KS) of both forms
    # (a tall last tile row runs the RW + 1 body; the RW body runs on the tile rows above it, if any)
    bodies = {(b.b3, b.nq, b.rw_last, b.ks) for c, b in br} | {(b.b3, b.nq, b.rw, b.ks) for c, b in br if not b.tall or b.tiles_y >= 2}
    assert bodies == {(b3, nq, rw, ks) for b3 in (False, True) for nq, rw, ks in ((4, 8, 3), (4, 9, 3), (2, 4, 3), (2, 5, 3), (4, 8, 1), (2, 4, 1))}


def test_the_production_rows_are_the_models_calls():
    """the (shape, window, flags) rows of the transforms at the reference width; the maps of a 512 x 1024 image and the next one up"""
    rows = {(c.ks, c.cin, c.cout, c.hp, c.wp, c.sphere, c.ring, c.ring_w, c.crop, c.shuffle, c.slope, c.res) for c in sc.PRODUCTION}
    for hp, wp in ((68, 132), (132, 260), (260, 516), (516, 1028)):
        assert (3, 192, 192, hp, wp, 1, 1, 2, 0, False, True, False) in rows and (3, 192, 192, hp, wp, 2, 2, 2, 0, False, True, True) in rows
    assert (3, 96, 96, 132, 260, 1, 2, 2, 0, False, True, False) in rows
    for hp, wp in ((132, 260), (260, 516)):
        assert (3, 192, 768, hp, wp, 1, 2, 2, 1, True, True, False) in rows and (1, 192, 768, hp, wp, 0, 2, 2, 1, True, False, True) in rows
    assert (1, 192, 96, 260, 516, 0, 2, 2, 0, False, True, False) in rows and (1, 96, 192, 260, 516, 0, 2, 2, 0, False, False, True) in rows
    # the rows recorded from CMP_Encoder / CMP_Decoder at 512 x 1024 (batch 8) that the lines above do not name
    for hp, wp in ((68, 132), (132, 260), (260, 516)):
        assert (3, 192, 192, hp, wp, 1, 2, 2, 0, False, False, False) in rows
    for hp, wp in ((36, 68), (68, 132)):
        assert (3, 192, 768, hp, wp, 1, 2, 2, 1, True, True, False) in rows and (1, 192, 768, hp, wp, 0, 2, 2, 1, True, False, True) in rows
    assert (1, 192, 96, 132, 260, 0, 2, 2, 0, False, True, False) in rows and (1, 96, 192, 132, 260, 0, 2, 2, 0, False, False, True) in rows
    assert all(c.n == 1 and c.pad in (0, 2) for c in sc.PRODUCTION)
    p = sc.PAST_4GIB
    plane = p.cin * p.hp * p.wp
    assert 10 * plane * 4 < 2 ** 32 < 11 * plane * 4 and 21 * plane < 2 ** 31 < 22 * plane and p.n == 22 and p.cout == p.cin


@pytest.mark.parametrize("tier", list(sc.TIERS))
def test_exact_domain_of_every_case(tier):
    """|b| + 4 |res| + sum |w||x| < 2^24 for every case in every tier it runs in, from the data as generated (the large production cases through
    their ranges: the same generator, and the bound only grows with cin and the kernel size, which the smaller maps share)"""
    xm, wm = sc.TIERS[tier]
    ran = 0
    for c in sc.CASES + [sc.PAST_4GIB]:
        if tier not in [t for _, t in sc.forms_of(c)]:
            continue
        assert (1 + 2.0 ** -7) ** 2 * c.cin * c.ks * c.ks * xm * wm + 8 + 4 * 8 < sc.EXACT_BELOW, c.name      # whatever the generator draws
        if _macs(c) <= MUTATION_MACS:
            data = sc.make_case(c, tier)
            bound = sc.assert_exact_domain(c, data, tier)
            assert float(np.abs(data["x"]).max()) <= xm and float(np.abs(data["w"]).max()) <= wm and bound > 0
            ran += 1
    assert ran >= len(sc.SMALL) - (1 if tier != "fp32" else 0)


def test_split_identities():
    """hi + lo holds every operand of every tier exactly, the dropped w_lo x_lo is zero, and each tier exercises the term it is there for"""
    v = np.arange(-65536, 65537, dtype=np.float32)
    hi, lo = sc.bf16_split(v)
    assert np.array_equal(hi + lo, v)                                       # every integer up to 2^16
    c = next(c for c in sc.SMALL if c.name == "s3_q4_low_pad3")
    for tier in sc.B3_TIERS:
        d = sc.make_case(c, tier)
        (xh, xl), (wh, wl) = sc.bf16_split(d["x"]), sc.bf16_split(d["w"])
        assert np.array_equal(xh + xl, d["x"]) and np.array_equal(wh + wl, d["w"])
        assert not (xl.any() and wl.any()), tier                            # w_lo x_lo == 0
        for lo, mine in ((xl, tier == "xlo"), (wl, tier == "wlo")):         # a tier's own operand needs its lo part in a good share of the cells, no other does
            assert (lo != 0).mean() > 0.4 if mine else not lo.any(), tier
    for tier, (xm, wm) in sc.TIERS.items():
        for m, is_lo in ((xm, tier == "xlo"), (wm, tier == "wlo")):
            assert (m > 256) == is_lo and m < 65536


def _small_forms():
    return [(c, tier) for c in MUTATED for tier in (["fp32"] + [t for b3, t in sc.forms_of(c) if t in ("xlo", "wlo")])]


@pytest.mark.parametrize("case,tier", _small_forms(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_mutation_changes_the_reference(case, tier):
    data = sc.make_case(case, tier)
    want = sc.reference(case, data)
    assert want.shape == sc.out_shape(case) and np.array_equal(want, want.astype(np.float32).astype(np.float64))
    frame = want == sc.SENTINEL
    assert frame.mean() < 1 and (frame.any() or case.crop == case.ring == case.ring_w)      # (a crop as wide as the ring leaves no frame)
    muts = [m for m, applies in sc.MUTATIONS.items() if applies(case, tier)]
    if tier != "fp32":
        muts = [m for m in muts if m.endswith("_lo_dropped")]              # the rest ran on the fp32 tier's data
    assert muts
    for m in muts:
        got = sc.reference(case, data, m)
        assert not np.array_equal(got, want), "%s / %s: mutation %s is invisible" % (case.name, tier, m)
    if tier == "xlo":                                                        # dropping x_lo changes a large share of the outputs, not a few (a slope of 0 hides an eighth; 32 channels of a 1x1 cancel now and then)
        assert (sc.reference(case, data, "x_lo_dropped") != want)[~frame].mean() > 0.25


def test_every_mutation_applies_somewhere():
    for m, applies in sc.MUTATIONS.items():
        assert any(applies(c, t) for c in MUTATED for _, t in sc.forms_of(c)), m


def test_reference_matches_the_oracle_on_a_sphere_case():
    """the reference's own sphere rule and convolution against the oracle's (pinned by tests/test_oracle_ops.py), on the two apron modes"""
    import oracle as orc
    for name in ("s3_q4_rem1", "s3_q4_low_pad3", "s3_q4_3rows_tall_pad1", "s3_q4_shuffle_768"):
        c = next(c for c in sc.SMALL if c.name == name)
        d = sc.make_case(c, "fp32")
        y = orc.conv2d(orc.sphere_pad_inplace(d["x"].copy(), c.pad), d["w"], d["b"], 1, 1)
        y = orc.prelu(y, d["slope"])[:, :, c.crop:c.hp - c.crop, c.crop:c.wp - c.crop]
        r0, r1, c0, c1 = c.ring - c.crop, c.hp - c.ring - c.crop, c.ring_w - c.crop, c.wp - c.ring_w - c.crop
        if c.shuffle:
            y, r0, r1, c0, c1 = orc.dtow(np.ascontiguousarray(y), 2, True), 2 * r0, 2 * r1, 2 * c0, 2 * c1
        assert np.array_equal(sc.reference(c, d)[:, :, r0:r1, c0:c1], y[:, :, r0:r1, c0:c1].astype(np.float64)), name


def test_describe_mismatch_names_the_tile():
    c = next(c for c in sc.SMALL if c.name == "s3_q4_3rows_tall_pad1")
    want = sc.reference(c, sc.make_case(c, "fp32"))
    got = want.copy()
    got[0, 100, 1 + 48, 1 + 17] += 1                                        # row 49 = the tall last tile row's ninth row of wave nh = 0... (ring 1)
    msg = sc.describe_mismatch(c, False, got, want)
    assert "tile (ty, tx) = (2, 1)" in msg and "wave (mq, nh) = (2, 1)" in msg and "accumulator m 0 row 7 (kq 1, v 0)" in msg and "{2: 1}" in msg, msg
    got = want.copy()
    got[0, 0, 0, 0] = 0
    assert "OUTSIDE the window" in sc.describe_mismatch(c, False, got, want)


def test_fusable_counts_tiles_as_the_launch_does(monkeypatch):
    """lic360_models._fusable restates sconv_launch's tile count; both against branch_of's, window heights 1 .. 80, both NQ"""
    import lic360_models as lm
    monkeypatch.setattr(lm.lic360, "sconv3x3_supported", lambda cin, cout: True)
    monkeypatch.setattr(lm, "FUSED_MIN_FILL", 0.0)

    class Conv(object):
        bias = True
        def __init__(self, cout):
            self.weight = torch.empty((cout, 32, 3, 3), device="meta")

    class Map(object):
        is_cuda, dtype, requires_grad = True, torch.float32, False
        def __init__(self, shape):
            self.shape = shape

    with torch.no_grad():
        for cout, nq in ((192, 4), (96, 2), (768, 4)):
            for nr in range(1, 81):
                for ring, ring_w, nc in ((2, 2, 40), (1, 2, 33)):
                    case = sc._c("t", 3, 32, cout, 3, nr + 2 * ring, nc + 2 * ring_w, ring=ring, ring_w=ring_w)
                    b = sc.branch_of(case, False)
                    tiles = case.n * b.tiles_y * b.tiles_x * b.blocks_y
                    assert sc.tile_rows(nr, nq)[0] == b.tiles_y
                    for thr, want in ((tiles, True), (tiles + 1, False)):
                        monkeypatch.setattr(lm, "FUSED_MIN_WORKGROUPS", thr)
                        assert lm._fusable(Conv(cout), Map((case.n, 32, case.hp, case.wp)), ring, ring_w) is want, (cout, nr, ring, ring_w, thr)


# ==== GDN
def test_gdn_cases_cover_every_kernel_and_edge():
    br = {sc.gdn_branch_of(c) for c in sc.GDN_CASES}
    assert br == {(ch // 16, vec) for ch in sc.GDN_CHANNELS for vec in (True, False)}
    ps = [(c, c.h * c.w) for c in sc.GDN_CASES]
    assert any(p % 2 == 1 for _, p in ps) and any(p % 4 == 2 for _, p in ps) and any(p % 4 == 0 and c.misaligned for c, p in ps)
    assert any(p < 64 for _, p in ps) and any(p % 64 == 0 and not c.prod for c, p in ps) and any(p % 64 == 1 for _, p in ps)
    assert {c.n for c in sc.GDN_CASES} >= {1, 3} and {c.inverse for c in sc.GDN_SMALL} == {True, False}
    for vec in (True, False):
        assert {c.inverse for c in sc.GDN_SMALL if sc.gdn_branch_of(c)[1] == vec} == {True, False}
    prod = {(c.c, c.h, c.w, c.inverse) for c in sc.GDN_PRODUCTION}
    assert prod == {(192, 68, 132, False), (192, 132, 260, False), (192, 260, 516, False), (192, 68, 132, True), (192, 132, 260, True),
                    (192, 260, 516, True), (192, 516, 1028, True)}


@pytest.mark.parametrize("case", sc.GDN_SMALL + sc.GDN_PRODUCTION[2:4], ids=lambda c: c.name)
def test_gdn_domain_and_mutations(case):
    data = sc.gdn_make(case)
    assert sc.gdn_assert_exact_domain(case, data) > 0
    assert 192 * 3 * 15 * 15 + 16 < sc.EXACT_BELOW                          # whatever the generator draws, at any size
    want = sc.gdn_reference(case, data)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    sq = sc.gdn_perfect_squares(data)
    assert sq.any(), "no cell with an integer norm"
    assert np.array_equal(want[sq], (data["x"] * np.sqrt(sc.gdn_sums(data)).astype(np.float32) if case.inverse else
                                     data["x"] / np.sqrt(sc.gdn_sums(data)).astype(np.float32))[sq])
    muts = [m for m, applies in sc.GDN_MUTATIONS.items() if applies(case)]
    for m in muts:
        assert not np.array_equal(sc.gdn_reference(case, data, m), want, equal_nan=True), "%s: mutation %s is invisible" % (case.name, m)


def test_every_gdn_mutation_applies_somewhere():
    for m, applies in sc.GDN_MUTATIONS.items():
        assert any(applies(c) for c in sc.GDN_SMALL), m
