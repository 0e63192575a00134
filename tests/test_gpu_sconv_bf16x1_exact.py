"""The single-pass bf16 ("bf16x1") sphere convolutions (lic360.sconv3x3_bf16x1 / sconv1x1_bf16x1; csrc/sconv_bf16x3.inc with NT = 1, kernels k_sconv_b1)
bit for bit, on every dispatch path: integer data on which the fp32-accumulated convolution of the bf16-rounded operands has one fp32 result whatever the
summation order (tests/sconv_bf16x1_cases.py), so the whole output tensor -- window and untouched frame (sentinel 7.0) in one comparison -- must EQUAL the
float64 reference.  Every case of the branch matrix and every production row in three tiers (hi: nothing rounds; xrnd / wrnd: x / w rounds up, down and
ties to both sides); every production row 20 times on two streams; 22 images at 516 x 1028 (image offsets past 2^32 bytes and 2^31 elements).
The only skip in this file is test_past_4gib's, taken when less than 32 GiB of device memory are free."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_bf16x1_cases as b1
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _fns(lic, case):
    name = "sconv%dx%d_bf16x1" % (case.ks, case.ks)
    return getattr(lic, name), getattr(lic, name + "_pack")


def _call(lic, case, data):
    """call(out) of a case on `data`: its entry point, device operands and keyword arguments"""
    conv, pack = _fns(lic, case)
    ops = (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"]))
    kw = dict(ring=case.ring, ring_w=case.ring_w, crop=case.crop, shuffle=case.shuffle)
    if case.ks == 3:
        kw.update(pad=case.pad, sphere=case.sphere)
    return lambda out: conv(*ops, out, **kw)


def _reference(case, tier, data):
    """a production case's xrnd reference is kept: shared with the repeatability test"""
    return gs.fp32_reference(lambda: b1.reference(case, data), ("sconv_bf16x1", case.name, tier) if case.prod and tier == "xrnd" else None)


def _describe(case):
    return lambda got, want: b1.describe_mismatch(case, True, got, want).replace("bf16x3", "bf16x1")


PARAMS = [(c, tier) for c in b1.CASES_B1 for tier in b1.TIERS]


@pytest.mark.parametrize("case,tier", PARAMS, ids=["%s-%s" % (c.name, t) for c, t in PARAMS])
def test_sconv_bf16x1_is_exact(lic, case, tier):
    assert getattr(lic, "sconv%dx%d_bf16x1_supported" % (case.ks, case.ks))(case.cin, case.cout)
    data = b1.make_case(case, tier)
    bound = b1.assert_exact_domain(case, data)
    want = _reference(case, tier, data)
    got = gs.sentinel_call(_call(lic, case, data), b1.out_shape(case), b1.SENTINEL)
    print("%s / %s: branch %s, |b| + 4 |res| + sum |w~||x~| <= %g" % (case.name, tier, tuple(b1.branch_of(case, True)), bound))
    gs.check_whole_output(got, want, _describe(case))


def test_the_pack_is_the_rounded_weight_in_operand_order(lic):
    """[blk][it = (cg ks + kw) ks + kh][mq][mt][lane = 16 kq + i] x 8 bf16 (csrc/sconv_bf16x3.inc, no hl index): each weight once, rounded to nearest even"""
    rng = np.random.default_rng(81)
    for ks, cin, cout in ((3, 64, 192), (1, 96, 96)):
        w = np.where(rng.random((cout, cin, ks, ks)) < 0.5, rng.standard_normal((cout, cin, ks, ks)),
                     b1._rounding_ints(rng, 1023, (cout, cin, ks, ks))).astype(np.float32)
        pk = getattr(lic, "sconv%dx%d_bf16x1_pack" % (ks, ks))(torch.from_numpy(w).cuda())
        assert pk.dtype == torch.bfloat16 and pk.numel() * 2 == cout * cin * ks * ks * 2
        nq = 4 if cout % 192 == 0 else 2
        got = pk.float().cpu().numpy().reshape(cout // (48 * nq), cin // 32 * ks * ks, nq, 3, 4, 16, 8)      # [blk][it][mq][mt][kq][i][j]
        ref = np.empty(got.shape, np.float32)
        for blk, it, mq, mt, kq, i in np.ndindex(*ref.shape[:6]):
            kh, kw, cg = it % ks, it // ks % ks, it // (ks * ks)
            ref[blk, it, mq, mt, kq, i] = w[blk * nq * 48 + 48 * mq + 16 * mt + i, 32 * cg + 8 * kq + np.arange(8), kh, kw]
        assert np.array_equal(got, b1.bf16_rne(ref))


REPEATS = [c for c in b1.CASES_B1 if c.prod]


@pytest.mark.parametrize("case", REPEATS, ids=[c.name for c in REPEATS])
def test_production_rows_repeat_bit_for_bit(lic, case):
    """20 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the reference"""
    data = b1.make_case(case, "xrnd")
    gs.repeat_on_two_streams(_call(lic, case, data), b1.out_shape(case), _reference(case, "xrnd", data), b1.SENTINEL, _describe(case))


def test_past_4gib(lic):
    """192 -> 192 at 516 x 1028, n = 22 (9 GB in, 9 GB out): image 10's planes straddle byte offset 2^32, image 21's element 2^31.  Images i and i + 11
    get the same input: they must give the same output, and no two others may; images 0 and 10 (and their twins) are compared with the float64 reference,
    the frame of every image with the sentinel."""
    gs.skip_below_free_memory(32)
    case = b1.PAST_4GIB
    c1 = case._replace(n=1)
    half = case.n // 2
    xm = b1.TIERS["xrnd"][0]
    data = b1.make_case(c1, "xrnd")                                         # w, b, slope (its one image is not used)
    b1.assert_exact_domain(c1, dict(data, x=np.full((1, case.cin, 1, 1), xm, np.float32)))
    x = gs.doubled(xm, 17, half, (case.cin, case.hp, case.wp))
    conv, pack = _fns(lic, case)
    out = torch.full(b1.out_shape(case), b1.SENTINEL, device="cuda:0")
    conv(x, pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), None, out, pad=case.pad, sphere=case.sphere, ring=case.ring, ring_w=case.ring_w)
    torch.cuda.synchronize()
    gs.pairs_check(out, "sconv3x3_bf16x1")
    assert gs.frame_is_untouched(out, case.ring, case.hp - case.ring, case.ring_w, case.wp - case.ring_w, b1.SENTINEL)
    for img in (0, half - 1):
        xi = x[img:img + 1].cpu().numpy()
        assert b1.rounding_classes(xi) == {"exact", "down", "up", "tie_down", "tie_up"}
        want = b1.reference(c1, dict(data, x=xi)).astype(np.float32)
        for i in (img, img + half):
            got = out[i:i + 1].cpu().numpy()
            assert np.array_equal(got, want), "image %d: %s" % (i, b1.describe_mismatch(c1, True, got, want))
