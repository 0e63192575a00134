"""tests/sconv_s2_cases.py checked by itself, without a GPU: the case list reaches every kernel instantiation and launch branch of the stride-2
sphere convolutions, the exactness condition holds for every case, the references can tell a wrong stride-2 kernel from a right one (each of a
list of plausible bugs changes the result on every case it applies to), and the reference is the reference model's own layers:
Conv2d(.., 3, stride 2, padding 3) resp. Conv2d(.., 1, stride 2, padding 2) behind SpherePad(2), interior against interior."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sconv_s2_cases as s2

# the mutation tests convolve on the CPU in float64: every small case and the production cases up to this many MACs per reference
MUTATION_MACS = 4e9


def _macs(c):
    oh, ow = s2.out_hw(c)
    return float(c.n) * c.cin * c.cout * c.ks * c.ks * oh * ow * 4         # (the stride-1 mutation convolves the whole input grid)


MUTATED = [c for c in s2.CASES if _macs(c) <= MUTATION_MACS]


def test_every_case_is_a_legal_call():
    """sconv_plan's stride-2 argument contract, restated: a case the native check would refuse tests nothing"""
    names = [c.name for c in s2.CASES]
    assert len(set(names)) == len(names)
    for c in s2.CASES:
        assert s2.supported(c.cin, c.cout, c.ks), c.name
        H, W = c.hp - 2 * c.pad, c.wp - 2 * c.pad
        assert H > 0 and W > 0 and H % 2 == 0 and W % 2 == 0 and c.oring >= 0 and c.sphere in (0, 1), c.name
        assert c.ks == 1 or c.pad >= 1, c.name
        assert not c.sphere or (c.ks == 3 and c.hp >= 4 * c.pad and c.wp >= 4 * c.pad), c.name
        assert 32.0 * c.hp * c.wp * 4 < 2.0 ** 32, c.name


def test_the_case_list_covers_the_branch_matrix():
    br = [(c, s2.branch_of(c)) for c in s2.CASES]
    missing = []

    def need(what, pred):
        if not any(pred(c, b) for c, b in br):
            missing.append(what)
    for ks in (3, 1):
        f = "%dx%d stride 2: " % (ks, ks)
        mine = lambda p, ks=ks: (lambda c, b: b.ks == ks and p(c, b))
        for nq in (4, 2):
            q = lambda p, nq=nq, mine=mine: mine(lambda c, b: b.nq == nq and p(c, b))
            need(f + "NQ = %d" % nq, q(lambda c, b: True))
            need(f + "NQ = %d, exactly one tile" % nq, q(lambda c, b: s2.out_hw(c) == (16, 16)))
            need(f + "NQ = %d, a window lower than one tile" % nq, q(lambda c, b: b.full == 0))
            need(f + "NQ = %d, a remainder on an extra tile row" % nq, q(lambda c, b: b.full >= 1 and b.rem > 0 and b.tiles_y == b.full + 1))
            need(f + "NQ = %d, 192 input channels" % nq, q(lambda c, b: c.cin == 192))
        need(f + "rows ragged", mine(lambda c, b: b.rem != 0))
        need(f + "columns ragged", mine(lambda c, b: s2.out_hw(c)[1] % 16 != 0))
        need(f + "columns exact", mine(lambda c, b: s2.out_hw(c)[1] % 16 == 0))
        need(f + "cout 384 (blockIdx.y 0 .. 1)", mine(lambda c, b: b.blocks_y == 2))
        need(f + "cout 96", mine(lambda c, b: c.cout == 96))
        need(f + "one chunk of input channels", mine(lambda c, b: b.chunks == 1))
        need(f + "32 input channels", mine(lambda c, b: c.cin == 32))
        need(f + "many chunks", mine(lambda c, b: b.chunks >= 6))
        for n in (1, 3):
            need(f + "n = %d" % n, mine(lambda c, b, n=n: c.n == n))
        for pad in (2, 3):
            need(f + "pad %d" % pad, mine(lambda c, b, pad=pad: c.pad == pad))
        for flag in (True, False):
            need(f + "slope %s" % flag, mine(lambda c, b, flag=flag: c.slope == flag))
            need(f + "residual %s" % flag, mine(lambda c, b, flag=flag: c.res == flag))
        if ks == 3:
            need(f + "cin 16", mine(lambda c, b: c.cin == 16))
            for sphere in (0, 1):
                need(f + "sphere %d" % sphere, mine(lambda c, b, sphere=sphere: c.sphere == sphere))
            need(f + "pad 3 under the sphere rule", mine(lambda c, b: c.sphere == 1 and c.pad == 3))
        need(f + "a production shape", mine(lambda c, b: c.prod))
    assert not missing, "the case list lost: " + "; ".join(missing)
    # every kernel instantiation sconv_launch can pick at stride 2: k_sconv3x3s2<NQ, RW, KS>
    assert {(b.nq, b.rw, b.ks) for c, b in br} == {(4, 8, 3), (2, 4, 3), (4, 8, 1), (2, 4, 1)}


def test_the_production_rows_are_the_models_calls():
    """the analysis transform at the reference width for a 512 x 1024 image: the hidden stages' conv1 (+ PReLU) and shortcut (+ the GDN branch),
    and SphereConv2; 128, 32 and 8 tiles per image"""
    rows = {(c.ks, c.cin, c.cout, c.hp, c.wp, c.pad, c.sphere, c.oring, c.slope, c.res) for c in s2.PRODUCTION}
    assert rows == {(3, 192, 192, 260, 516, 2, 1, 2, True, False), (3, 192, 192, 132, 260, 2, 1, 2, True, False), (3, 192, 192, 68, 132, 2, 1, 2, False, False),
                    (1, 192, 192, 260, 516, 2, 0, 2, False, True), (1, 192, 192, 132, 260, 2, 0, 2, False, True)}
    assert all(c.n == 1 and c.prod for c in s2.PRODUCTION)
    tiles = [b.tiles_y * b.tiles_x for b in map(s2.branch_of, s2.PRODUCTION[:3])]
    assert tiles == [128, 32, 8] and all(s2.out_hw(c)[0] % 16 == 0 and s2.out_hw(c)[1] % 16 == 0 for c in s2.PRODUCTION)


def test_exact_domain_of_every_case():
    """|b| + 4 |res| + sum |w||x| < 2^24 for every case, from the data as generated (the large production cases through their ranges: the same
    generator, and the bound grows with cin and the kernel size only); at 192 channels in the fp32 tier: 192 * 9 * 4 * 8 = 55 296"""
    xm, wm = s2.TIERS["fp32"]
    ran = 0
    for c in s2.CASES:
        assert c.cin * c.ks * c.ks * xm * wm + 8 + 4 * 8 < float(1 << 24), c.name
        if _macs(c) <= MUTATION_MACS:
            data = s2.make_case(c)
            bound = s2.assert_exact_domain(c, data, "fp32")
            assert float(np.abs(data["x"]).max()) <= xm and float(np.abs(data["w"]).max()) <= wm and 0 < bound < float(1 << 24)
            ran += 1
    assert ran >= len(s2.SMALL)
    assert 192 * 9 * 4 * 8 == 55296


@pytest.mark.parametrize("case", MUTATED, ids=lambda c: c.name)
def test_every_mutation_changes_the_reference(case):
    data = s2.make_case(case)
    want = s2.reference(case, data)
    assert want.shape == s2.out_shape(case) and np.array_equal(want, want.astype(np.float32).astype(np.float64))       # the expected values are fp32 numbers
    frame = want == s2.SENTINEL
    r, (oh, ow) = case.oring, s2.out_hw(case)
    assert frame.mean() < 1 and (case.oring == 0 or frame[:, :, :r].all() and frame[:, :, r + oh:].all() and frame[:, :, :, :r].all() and frame[:, :, :, r + ow:].all())
    muts = [m for m, applies in s2.MUTATIONS.items() if applies(case)]
    assert len(muts) >= 8
    for m in muts:
        got = s2.reference(case, data, m)
        assert got.shape == want.shape and not np.array_equal(got, want), "%s: mutation %s is invisible" % (case.name, m)
    for m in ("taps_on_2i_plus_1", "stride_rows_only", "stride_cols_only", "stride_1_read"):      # a wrong stride changes most of the window, not a few cells
        assert (s2.reference(case, data, m) != want)[~frame].mean() > 0.25, m


def test_every_mutation_applies_somewhere():
    for m, applies in s2.MUTATIONS.items():
        for ks in (3, 1):
            if ks == 1 and m in ("pole_no_mirror", "wrap_off_by_one", "kh_kw_swapped"):
                continue
            assert any(applies(c) for c in MUTATED if c.ks == ks), (m, ks)


def _sphere_pad(x, pad):
    """SpherePad(pad) applied to a copy of x: every apron cell from the interior by the sphere rule"""
    sh, sw = s2.source_cells(x.shape[2], x.shape[3], pad, 1)
    return np.ascontiguousarray(x[:, :, sh, sw])


@pytest.mark.parametrize("name", ["d3_q4_one_tile", "d3_q4_rows_n3", "d3_q2_one_tile_cin16", "d3_q4_384_rem1", "d1_q4_one_tile", "d1_q2_ragged", "d1_q4_low"])
def test_reference_is_the_reference_models_layer(name):
    """F.conv2d(SpherePad(2)(x), w, b, 2, 3) and (.., 2, 2): Conv2d(cin, c, 3, 2, 3) and Conv2d(cin, c, 1, 2, 2) of ResidualBlockDown / SphereConv2 on
    the padded map, interior against interior (their outputs carry a 2-cell apron: the interior starts at (2, 2)); and the oracle's own pad + conv"""
    import oracle as orc
    c = next(c for c in s2.SMALL if c.name == name)
    assert c.pad == 2
    d = s2.make_case(c)
    oh, ow = s2.out_hw(c)
    xp = _sphere_pad(d["x"], 2) if c.ks == 3 else d["x"]                   # (the shortcut runs before the pad and reads the interior only)
    y = F.conv2d(torch.from_numpy(xp).double(), torch.from_numpy(d["w"]).double(), torch.from_numpy(d["b"]).double(), 2, 3 if c.ks == 3 else 2).numpy()
    assert y.shape[2:] == (oh + 4, ow + 4)
    yo = orc.conv2d(orc.sphere_pad_inplace(d["x"].copy(), 2) if c.ks == 3 else d["x"], d["w"], d["b"], 2, 3 if c.ks == 3 else 2).astype(np.float64)
    assert np.array_equal(yo[:, :, 2:2 + oh, 2:2 + ow], y[:, :, 2:2 + oh, 2:2 + ow])
    if d["slope"] is not None:
        y = np.where(y > 0, y, y * d["slope"].astype(np.float64)[None, :, None, None])
    y = y[:, :, 2:2 + oh, 2:2 + ow]
    if d["res"] is not None:
        y = y + d["res"][:, :, c.oring:c.oring + oh, c.oring:c.oring + ow]
    assert np.array_equal(s2.reference(c, d)[:, :, c.oring:c.oring + oh, c.oring:c.oring + ow], y), name


def test_describe_mismatch_names_the_tile():
    c = next(c for c in s2.SMALL if c.name == "d3_q4_rows_n3")
    want = s2.reference(c, s2.make_case(c))
    got = want.copy()
    got[1, 100, 2 + 19, 2 + 5] += 1                                         # output (19, 5): second tile row, its row 3 = wave nh 0 row 3; channel 100 = mq 2, m 0, kq 1, v 0
    msg = s2.describe_mismatch(c, got, want)
    assert "tile (ty, tx) = (1, 0)" in msg and "wave (mq, nh) = (2, 0)" in msg and "accumulator m 0 row 3 (kq 1, v 0)" in msg and "{1: 1}" in msg, msg
    got = want.copy()
    got[0, 0, 0, 0] = 0
    assert "OUTSIDE the window" in s2.describe_mismatch(c, got, want)


def test_fusable_s2_counts_tiles_on_the_output_window(monkeypatch):
    """lic360_models._fusable_s2 restates sconv_plan's stride-2 tile count, on the OUTPUT window; odd interiors never go fused"""
    import lic360_models as lm
    monkeypatch.setattr(lm.lic360, "sconv3x3s2_supported", lambda cin, cout: True)
    monkeypatch.setattr(lm.lic360, "sconv1x1s2_supported", lambda cin, cout: True)

    class Conv(object):
        bias = True
        def __init__(self, cout, ks):
            self.weight, self.kernel_size = torch.empty((cout, 32, ks, ks), device="meta"), (ks, ks)

    class Map(object):
        is_cuda, dtype, requires_grad = True, torch.float32, False
        def __init__(self, shape):
            self.shape = shape
        def is_contiguous(self):
            return True

    with torch.no_grad():
        for ks in (3, 1):
            for cout in (192, 96, 384):
                for oh in range(1, 50):
                    case = s2._c("t", ks, 32, cout, 3, oh, 21)
                    b = s2.branch_of(case)
                    tiles = case.n * b.tiles_y * b.tiles_x * b.blocks_y
                    for thr, want in ((tiles, True), (tiles + 1, False)):
                        monkeypatch.setattr(lm, "FUSED_S2_MIN_WORKGROUPS", thr)
                        assert lm._fusable_s2(Conv(cout, ks), Map((case.n, 32, case.hp, case.wp))) is want, (ks, cout, oh, thr)
                monkeypatch.setattr(lm, "FUSED_S2_MIN_WORKGROUPS", 0)
                assert lm._fusable_s2(Conv(cout, ks), Map((1, 32, 4 + 31, 4 + 32))) is False
        # the committed thresholds: from 128 tiles, one round of the 256 CUs as it is, further rounds filled to FUSED_MIN_FILL (n tiles: n images of one tile)
        monkeypatch.undo()
        monkeypatch.setattr(lm.lic360, "sconv3x3s2_supported", lambda cin, cout: True)
        assert lm.FUSED_S2_MIN_WORKGROUPS == 128 and lm.FUSED_MIN_FILL == 0.8
        for tiles, want in ((64, False), (127, False), (128, True), (256, True), (288, False), (409, False), (410, True), (512, True), (1024, True)):
            assert lm._fusable_s2(Conv(192, 3), Map((tiles, 32, 36, 36))) is want, tiles
        # the analysis transform at the reference width, 512 x 1024: stages 2 and 3 go native at batch 8, SphereConv2 (8 tiles per image) from batch 16
        for n, want in ((1, (True, False, False)), (2, (True, False, False)), (8, (True, True, False)), (16, (True, True, True))):
            assert tuple(lm._fusable_s2(Conv(192, 3), Map((n, 192, hp, wp))) for hp, wp in ((260, 516), (132, 260), (68, 132))) == want, n
