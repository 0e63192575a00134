"""The single-pass bf16 forms of the stride-2 sphere convolutions (lic360.sconv3x3s2_bf16x1 / sconv1x1s2_bf16x1; kernels k_sconv_b1s2) bit for bit:
integer data on which the convolution of the ROUNDED operands has one fp32 result whatever the summation order (tests/sconv_s2_bf16x1_cases.py), so the
whole output tensor -- the interior window and the untouched frame in one comparison -- must EQUAL a float64 reference.  Every case in three tiers (nothing
rounds / x rounds / w rounds); the five calls the analysis transform makes at the reference width 20 times on two streams; the operand checks.
There is no skip in this file: without a HIP device its tests fail."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_s2_bf16x1_cases as sb
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _operands(lic, case, data):
    """the call, its device operands (everything but `out`) and keyword arguments; the weight travels in the STRIDE-1 bf16x1 pack"""
    conv, pack = (lic.sconv3x3s2_bf16x1, lic.sconv3x3_bf16x1_pack) if case.ks == 3 else (lic.sconv1x1s2_bf16x1, lic.sconv1x1_bf16x1_pack)
    kw = dict(pad=case.pad, oring=case.oring)
    if case.ks == 3:
        kw.update(sphere=bool(case.sphere))
    return conv, (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"])), kw


def _call(lic, case, data):
    conv, ops, kw = _operands(lic, case, data)
    return lambda out: conv(*ops, out, **kw)


def _reference(case, tier, data):
    """a production case's xrnd reference is kept: shared with the repeatability test"""
    return gs.fp32_reference(lambda: sb.reference(case, data), ("sconv_s2_bf16x1", case.name, tier) if case.prod and tier == "xrnd" else None)


@pytest.mark.parametrize("tier", list(sb.TIERS))
@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: c.name)
def test_sconv_s2_bf16x1_is_exact(lic, case, tier):
    assert (lic.sconv3x3s2_bf16x1_supported if case.ks == 3 else lic.sconv1x1s2_bf16x1_supported)(case.cin, case.cout)
    data = sb.make_case(case, tier)
    bound = sb.assert_exact_domain(case, data)
    want = _reference(case, tier, data)
    got = gs.sentinel_call(_call(lic, case, data), sb.out_shape(case), sb.SENTINEL)
    print("%s / %s: branch %s, |b| + 4 |res| + sum |w~||x~| <= %g" % (case.name, tier, tuple(sb.branch_of(case)), bound))
    gs.check_whole_output(got, want, lambda g, w: sb.describe_mismatch(case, g, w))


def test_a_fresh_out_is_zero_filled(lic):
    """without `out`: the interior window in a map of zeros (SphereTrim applied)"""
    case = next(c for c in sb.SMALL if c.name == "d3_q4_one_tile")
    data = sb.make_case(case, "xrnd")
    assert case.oring == 2
    frame = np.ones(sb.out_shape(case), bool)
    frame[:, :, 2:-2, 2:-2] = False
    want = np.where(frame, np.float32(0), _reference(case, "xrnd", data))
    conv, ops, kw = _operands(lic, case, data)
    got = conv(*ops, **kw).cpu().numpy()
    assert np.array_equal(got, want), sb.describe_mismatch(case, got, want)


@pytest.mark.parametrize("case", sb.PRODUCTION, ids=lambda c: c.name)
def test_production_cases_repeat_bit_for_bit(lic, case):
    """20 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the
    reference.  Determinism under ordinary use (two streams, ordinary arguments); stops at the first difference."""
    data = sb.make_case(case, "xrnd")
    gs.repeat_on_two_streams(_call(lic, case, data), sb.out_shape(case), _reference(case, "xrnd", data), sb.SENTINEL,
                             lambda g, w: sb.describe_mismatch(case, g, w))


def test_operand_checks_refuse_before_the_kernel(lic):
    """the package's operand checks on the down-sampled shapes: a wrong `out` or `residual`, an odd interior, a short pack and an fp32 pack are errors,
    not out-of-bounds device accesses"""
    for name in ("d3_q4_one_tile", "d1_q4_one_tile"):
        case = next(c for c in sb.SMALL if c.name == name)
        data = sb.make_case(case, "hi")
        conv, ops, kw = _operands(lic, case, data)
        x, packed, b, slope, _ = ops
        with pytest.raises(lic.Lic360Error):
            conv(x, packed, b, slope, None, torch.empty((1, 192, 36, 36), device="cuda:0"), **kw)     # the input's shape, not the output's
        with pytest.raises(lic.Lic360Error):
            conv(x, packed, b, slope, torch.empty((1, 192, 36, 36), device="cuda:0"), None, **kw)
        with pytest.raises(lic.Lic360Error):
            conv(x[:, :, :-1].contiguous(), packed, b, slope, None, None, **kw)                         # an odd interior
        with pytest.raises(lic.Lic360Error):
            conv(x, packed[:-8], b, slope, None, None, **kw)                                            # a short pack
        fp32_pack = (lic.sconv3x3_pack if case.ks == 3 else lic.sconv1x1_pack)(gs.dev(data["w"]))
        with pytest.raises(lic.Lic360Error):
            conv(x, fp32_pack, b, slope, None, None, **kw)                                              # the fp32 stride-2 form's pack
        with pytest.raises(lic.Lic360Error):
            conv(x, packed.float(), b, slope, None, None, **kw)
