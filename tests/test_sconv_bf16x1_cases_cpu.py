"""tests/sconv_bf16x1_cases.py checked by itself, without a GPU: its bit-level round-to-nearest-even against torch.bfloat16 (random floats, ties, the
named integers); the case list reaches every bf16x1 body instantiation; the exactness condition holds for every case and tier, on the rounded operands;
every rounding tier of every case holds values that round up, round down and tie to both sides; and the reference can tell a wrong kernel from a right
one -- each plausible arithmetic bug of this form (truncation, half-away rounding, an operand left unrounded, the lo term added, bias or residual
rounded), and each geometry bug of tests/sconv_cases.py applied behind the rounding, changes the result on the tier meant to catch it."""
import numpy as np
import pytest
import torch

import sconv_bf16x1_cases as b1
import sconv_cases as sc

MUTATION_MACS = 4e9                                                        # as tests/test_sconv_cases_cpu.py: the production cases above it differ in map size only


def _macs(c):
    return float(c.n) * c.cin * c.cout * c.ks * c.ks * c.hp * c.wp


MUTATED = [c for c in b1.CASES_B1 if _macs(c) <= MUTATION_MACS]


def _torch_bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).bfloat16().float().numpy()


def test_bit_level_rounding_is_torch_bfloat16s():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(200000).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 7, 200000).astype(np.float32),
                        np.arange(-70000, 70001, dtype=np.float32), np.float32([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** 100])])
    assert np.array_equal(b1.bf16_rne(v).view(np.uint32), _torch_bf16(v).view(np.uint32))
    # ties: every float32 exactly halfway between two bf16 numbers (low half = 0x8000), a sample over exponents and both signs
    hi = rng.integers(0x0080, 0x7F00, 100000).astype(np.uint32)            # normal, finite, below the last binade
    ties = np.concatenate([(hi << np.uint32(16)) | np.uint32(0x8000), (hi << np.uint32(16)) | np.uint32(0x80008000)]).view(np.float32)
    got = b1.bf16_rne(ties)
    assert np.array_equal(got.view(np.uint32), _torch_bf16(ties).view(np.uint32))
    assert not ((got.view(np.uint32) >> np.uint32(16)) & np.uint32(1)).any()                       # every tie went to the even neighbour
    assert np.array_equal(b1.bf16_half_away(ties).view(np.uint32) >> np.uint32(16), (ties.view(np.uint32) >> np.uint32(16)) + np.uint32(1))
    assert np.array_equal(b1.bf16_truncate(ties).view(np.uint32) >> np.uint32(16), ties.view(np.uint32) >> np.uint32(16))


def test_the_named_integers_round_as_stated():
    pairs = ((257, 256), (259, 260), (261, 260), (263, 264), (513, 512), (2047, 2048))
    for v, want in pairs:
        for s in (1.0, -1.0):
            assert float(b1.bf16_rne(np.float32([s * v]))[0]) == s * want, (s * v, want)
            assert float(_torch_bf16(np.float32([s * v]))[0]) == s * want
    for name, values in b1.ROUNDS.items():
        for v in values:
            for s in (1.0, -1.0):
                assert b1.rounding_classes(np.float32([s * v])) == {name}, (name, s * v)
    assert b1.rounding_classes(np.arange(-256, 257, dtype=np.float32)) == {"exact"}
    pool = {m for ms in b1.ROUNDS.values() for m in ms}
    assert {257, 259, 261, 263, 513, 2047} <= pool and max(pool) <= 2047
    assert all(any(m <= 1023 for m in ms) for ms in b1.ROUNDS.values())                           # the weight tier's bound reaches every class too


def test_the_case_list_reaches_every_bf16x1_body():
    br = [(c, b1.branch_of(c, True)) for c in b1.CASES_B1]
    assert len(br) >= 40 and all(sc.supported(True, c.cin, c.cout, c.ks) for c, _ in br)
    # a tall last tile row runs the RW + 1 body; the RW body runs on the tile rows above it, if any
    bodies = {(b.nq, b.rw_last, b.ks) for c, b in br} | {(b.nq, b.rw, b.ks) for c, b in br if not b.tall or b.tiles_y >= 2}
    assert bodies == b1.BODIES
    assert any(c.prod for c, _ in br) and b1.PAST_4GIB.n == 22 and sc.supported(True, b1.PAST_4GIB.cin, b1.PAST_4GIB.cout, 3)
    have = lambda p: any(p(c, b) for c, b in br)
    for ks in (3, 1):
        for what, p in (("one chunk", lambda c, b: b.chunks == 1), ("six chunks", lambda c, b: b.chunks == 6), ("blockIdx.y up to 3", lambda c, b: b.blocks_y == 4),
                        ("shuffle with residual", lambda c, b: c.shuffle and c.res), ("crop without shuffle", lambda c, b: c.crop == 1 and not c.shuffle),
                        ("n = 3", lambda c, b: c.n == 3), ("no slope", lambda c, b: not c.slope), ("ragged columns", lambda c, b: (c.wp - 2 * c.ring_w) % 16 != 0)):
            assert have(lambda c, b, p=p, ks=ks: b.ks == ks and p(c, b)), (ks, what)
    for sphere in (0, 1, 2):
        assert have(lambda c, b: c.ks == 3 and c.sphere == sphere), sphere


@pytest.mark.parametrize("tier", list(b1.TIERS))
def test_exact_domain_and_rounding_classes_of_every_case(tier):
    """|b| + 4 |res| + sum |w~||x~| < 2^24 for every case, from the data as generated (the large production cases through their ranges: rounding moves a
    magnitude up by at most 2^-8 of itself), and the tier's own operand holds every rounding class while the other operand needs no rounding"""
    xm, wm = b1.TIERS[tier]
    ran = 0
    for c in b1.CASES_B1 + [b1.PAST_4GIB]:
        assert (1 + 2.0 ** -8) ** 2 * c.cin * c.ks * c.ks * xm * wm + 5 * b1.EPILOGUE_MAX < b1.EXACT_BELOW, c.name
        if _macs(c) > MUTATION_MACS:
            continue
        data = b1.make_case(c, tier)
        bound = b1.assert_exact_domain(c, data)
        assert float(np.abs(data["x"]).max()) <= xm and float(np.abs(data["w"]).max()) <= wm and bound > 0
        interior = data["x"][:, :, c.pad:c.hp - c.pad, c.pad:c.wp - c.pad] if c.pad else data["x"]      # (a sphere rule never reads the apron)
        cx, cw = b1.rounding_classes(interior), b1.rounding_classes(data["w"])
        allc = {"exact", "down", "up", "tie_down", "tie_up"}
        assert cx == (allc if tier == "xrnd" else {"exact"}), (c.name, tier, cx)
        assert cw == (allc if tier == "wrnd" else {"exact"}), (c.name, tier, cw)
        assert (b1.bf16_rne(data["b"]) != data["b"]).mean() > 0.25, c.name                            # most biases are not bf16 numbers
        assert data["res"] is None or (b1.bf16_rne(data["res"]) != data["res"]).mean() > 0.25
        ran += 1
    assert ran >= len([c for c in sc.SMALL if sc.supported(True, c.cin, c.cout, c.ks)])


def _forms():
    return [(c, t) for c in MUTATED for t in b1.TIERS]


@pytest.mark.parametrize("case,tier", _forms(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_every_mutation_changes_the_reference(case, tier):
    data = b1.make_case(case, tier)
    want = b1.reference(case, data)
    assert want.shape == b1.out_shape(case) and np.array_equal(want, want.astype(np.float32).astype(np.float64))
    frame = want == b1.SENTINEL
    assert frame.mean() < 1 and (frame.any() or case.crop == case.ring == case.ring_w)
    muts = [m for m, applies in b1.MUTATIONS.items() if applies(case, tier)]
    if tier != "hi":
        muts = [m for m in muts if m in b1.ARITHMETIC_MUTATIONS]           # the geometry mutations ran on the hi tier's data
    assert muts
    for m in muts:
        got = b1.reference(case, data, m)
        assert not np.array_equal(got, want), "%s / %s: mutation %s is invisible" % (case.name, tier, m)
    if tier == "hi":                                                        # nothing rounds: the form's result is the exact convolution
        assert np.array_equal(want, sc.reference(case, data)) and np.array_equal(want, b1.reference(case, data, "truncation"))
    else:                                                                   # rounding changes a large share of the outputs, not a few
        assert (b1.reference(case, data, "lo_added") != want)[~frame].mean() > 0.25


def test_every_mutation_applies_somewhere():
    for m, applies in b1.MUTATIONS.items():
        assert any(applies(c, t) for c in MUTATED for t in b1.TIERS), m
    assert set(b1.ARITHMETIC_MUTATIONS) == {"truncation", "half_away", "x_not_rounded", "w_not_rounded", "lo_added", "bias_rounded", "res_rounded"}
    for t, muts in (("xrnd", {"truncation", "half_away", "x_not_rounded", "lo_added"}), ("wrnd", {"truncation", "half_away", "w_not_rounded", "lo_added"})):
        assert muts <= {m for m, applies in b1.ARITHMETIC_MUTATIONS.items() if applies(MUTATED[0], t)}


def test_the_reference_is_the_float64_convolution_of_torch_rounded_operands():
    """the reference against an independent statement: torch.bfloat16 rounding and torch's float64 conv2d over the sphere-padded map (the oracle's pad)"""
    import oracle as orc
    import torch.nn.functional as F
    for name in ("s3_q4_rem1", "s3_q4_low_pad3"):
        c = next(c for c in sc.SMALL if c.name == name)
        for tier in ("xrnd", "wrnd"):
            d = b1.make_case(c, tier)
            xp = orc.sphere_pad_inplace(_torch_bf16(d["x"]).copy(), c.pad)
            y = F.conv2d(torch.from_numpy(xp).double(), torch.from_numpy(_torch_bf16(d["w"])).double(), torch.from_numpy(d["b"]).double(), 1, 1).numpy()
            y = np.where(y > 0, y, y * d["slope"].astype(np.float64)[None, :, None, None])
            r0, r1, c0, c1 = c.ring, c.hp - c.ring, c.ring_w, c.wp - c.ring_w
            assert np.array_equal(b1.reference(c, d)[:, :, r0:r1, c0:c1], y[:, :, r0:r1, c0:c1]), (name, tier)
