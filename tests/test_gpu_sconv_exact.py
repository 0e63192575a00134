"""The sphere convolutions (csrc/conv3x3_kernels.hip, csrc/sconv_bf16x3.inc) bit for bit, on every dispatch path: integer data on which a
convolution has one fp32 result whatever the summation order (tests/sconv_cases.py), so the whole output tensor -- window and untouched frame in
one comparison -- must EQUAL a float64 reference.  The branch matrix on small maps and the shapes the models run, each in the fp32 form and, where
the split-bf16 form takes the shape, in its three tiers (hi / xlo / wlo: which of the three products carries the data); 22 images at 516 x 1028
(9 GB in, 9 GB out: image offsets past 2^32 bytes and 2^31 elements); every production case 20 times on two streams.

bf16x3: v_mfma_f32_16x16x32_bf16 was found (on an MI355X, by these tests) to add its 32 products and the accumulator exactly when all of them are
integers below 2^24: the three tiers pass at bounds sum |w||x| up to 7.1e6, and test_bf16_mfma_adds_integers_exactly_up_to_2_24 drives all-positive
operands to sums of 1.29e7.  So the exactness bound of the tiers is k = 24, the fp32 form's (DESIGN.md 7c').
The only skip in this file is test_past_4gib's, taken when less than 32 GiB of device memory are free."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_cases as sc
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _fns(lic, case, b3):
    name = "sconv%dx%d%s" % (case.ks, case.ks, "_bf16x3" if b3 else "")
    return getattr(lic, name), getattr(lic, name + "_pack")


def _call(lic, case, b3, data):
    """call(out) of a case on `data`: its entry point, device operands and keyword arguments"""
    conv, pack = _fns(lic, case, b3)
    ops = (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"]))
    kw = dict(ring=case.ring, ring_w=case.ring_w, crop=case.crop, shuffle=case.shuffle)
    if case.ks == 3:
        kw.update(pad=case.pad, sphere=case.sphere)
    return lambda out: conv(*ops, out, **kw)


def _reference(case, tier, data):
    """a production case's fp32 / xlo reference is kept: shared with the repeatability test"""
    return gs.fp32_reference(lambda: sc.reference(case, data), ("sconv", case.name, tier) if case.prod and tier in ("fp32", "xlo") else None)


PARAMS = [(c, b3, tier) for c in sc.CASES for b3, tier in sc.forms_of(c)]


@pytest.mark.parametrize("case,b3,tier", PARAMS, ids=["%s-%s" % (c.name, t) for c, b3, t in PARAMS])
def test_sconv_is_exact(lic, case, b3, tier):
    assert getattr(lic, "sconv%dx%d%s_supported" % (case.ks, case.ks, "_bf16x3" if b3 else ""))(case.cin, case.cout)
    data = sc.make_case(case, tier)
    bound = sc.assert_exact_domain(case, data, tier)
    want = _reference(case, tier, data)
    got = gs.sentinel_call(_call(lic, case, b3, data), sc.out_shape(case), sc.SENTINEL)
    print("%s / %s: branch %s, |b| + 4 |res| + sum |w||x| <= %g" % (case.name, tier, tuple(sc.branch_of(case, b3)), bound))
    gs.check_whole_output(got, want, lambda g, w: sc.describe_mismatch(case, b3, g, w))


@pytest.mark.parametrize("ks", [3, 1])
def test_bf16_mfma_adds_integers_exactly_up_to_2_24(lic, ks):
    """what the guides state for the fp32 MFMA only: does v_mfma_f32_16x16x32_bf16 add its 32 products and the accumulator exactly when all are
    integers below 2^24?  The tiers' random signs keep their running sums far below their bound; here every operand is positive (3x3: x in
    192 .. 255, w in 30 .. 36, 192 channels: sums grow monotonically to about 1.27e7, bound 1.59e7 < 2^24 = 1.68e7; 1x1: x and w in 224 .. 255, sums to
    about 1.1e7), so the accumulator passes through every magnitude up to there on its way and ends above 2^23."""
    case = sc._c("b3_adder_%d" % ks, ks, 192, 192, 1, 24, 40, slope=False)
    rng = np.random.default_rng(ks)
    xlo, wlo, whi = (192, 30, 36) if ks == 3 else (224, 224, 255)
    data = dict(x=rng.integers(xlo, 256, (1, 192, 24, 40)).astype(np.float32), w=rng.integers(wlo, whi + 1, (192, 192, ks, ks)).astype(np.float32),
                b=np.zeros(192, np.float32), slope=None, res=None)
    assert all(not p[1].any() for p in (sc.bf16_split(data["x"]), sc.bf16_split(data["w"])))     # 8 significant bits: the hi product alone
    bound = sc.assert_exact_domain(case, data, "hi")
    want = gs.fp32_reference(lambda: sc.reference(case, data))
    win = want[:, :, 2:-2, 2:-2]
    print("bf16 MFMA adder probe %dx%d: sums %g .. %g, bound %g" % (ks, ks, win.min(), win.max(), bound))
    assert win.min() > 2.0 ** 23 and bound < sc.EXACT_BELOW
    got = gs.sentinel_call(_call(lic, case, True, data), sc.out_shape(case), sc.SENTINEL)
    gs.check_whole_output(got, want, lambda g, w: sc.describe_mismatch(case, True, g, w))


REPEATS = [(c, b3, tier) for c in sc.PRODUCTION for b3, tier in sc.forms_of(c) if tier in ("fp32", "xlo")]


@pytest.mark.parametrize("case,b3,tier", REPEATS, ids=["%s-%s" % (c.name, t) for c, b3, t in REPEATS])
def test_production_cases_repeat_bit_for_bit(lic, case, b3, tier):
    """20 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the
    reference.  Determinism under ordinary use (two streams, ordinary arguments); stops at the first difference."""
    data = sc.make_case(case, tier)
    gs.repeat_on_two_streams(_call(lic, case, b3, data), sc.out_shape(case), _reference(case, tier, data), sc.SENTINEL,
                             lambda g, w: sc.describe_mismatch(case, b3, g, w))


def test_past_4gib(lic):
    """192 -> 192 at 516 x 1028, n = 22: image 10's planes straddle byte offset 2^32, image 21's element 2^31.  Images i and i + 11 get the same
    input: they must give the same output, and no two others may; images 0, 10 and 21 are compared with the float64 reference, the frame of every
    image with the sentinel.  Then gdn_forward on a tensor of the same shape, checked the same way."""
    gs.skip_below_free_memory(32)
    case = sc.PAST_4GIB
    c1 = case._replace(n=1)
    half = case.n // 2
    for b3, tier in ((False, "fp32"), (True, "xlo")):
        data = sc.make_case(c1, tier)                                       # w, b, slope (its one image is not used)
        sc.assert_exact_domain(c1, dict(data, x=np.full((1, case.cin, 1, 1), sc.TIERS[tier][0], np.float32)), tier)
        x = gs.doubled(sc.TIERS[tier][0], 11 + b3, half, (case.cin, case.hp, case.wp))
        conv, pack = _fns(lic, case, b3)
        out = torch.full(sc.out_shape(case), sc.SENTINEL, device="cuda:0")
        conv(x, pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), None, out, pad=case.pad, sphere=case.sphere, ring=case.ring, ring_w=case.ring_w)
        torch.cuda.synchronize()
        gs.pairs_check(out, "sconv3x3" + ("_bf16x3" if b3 else ""))
        assert gs.frame_is_untouched(out, case.ring, case.hp - case.ring, case.ring_w, case.wp - case.ring_w, sc.SENTINEL)
        for img in (0, half - 1):
            want = sc.reference(c1, dict(data, x=x[img:img + 1].cpu().numpy())).astype(np.float32)
            for i in (img, img + half):
                got = out[i:i + 1].cpu().numpy()
                assert np.array_equal(got, want), "image %d: %s" % (i, sc.describe_mismatch(c1, b3, got, want))
        del x, out
    torch.cuda.empty_cache()
    gcase = sc.GdnCase("past_4gib", case.cin, case.n, case.hp, case.wp, False, False, True)
    gdata = sc.gdn_make(gcase, n=1)
    x = gs.doubled(15, 13, half, (case.cin, case.hp, case.wp))
    out = lic.gdn_forward(x, gs.dev(gdata["gamma"]), gs.dev(gdata["beta"]))
    torch.cuda.synchronize()
    gs.pairs_check(out, "gdn_forward")
    for img in (0, half - 1):
        want = sc.gdn_reference(gcase, dict(gdata, x=x[img:img + 1].cpu().numpy()))
        for i in (img, img + half):
            assert np.array_equal(out[i:i + 1].cpu().numpy(), want), "gdn_forward: image %d" % i
