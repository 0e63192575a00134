"""The single-pass bf16 forms of the stride-2 sphere convolutions (lic360.sconv3x3s2_bf16x1 / sconv1x1s2_bf16x1; kernels k_sconv_b1s2) bit for bit:
integer data on which the convolution of the ROUNDED operands has one fp32 result whatever the summation order (tests/sconv_s2_bf16x1_cases.py), so the
whole output tensor -- the interior window and the untouched frame in one comparison -- must EQUAL a float64 reference.  Every case in three tiers (nothing
rounds / x rounds / w rounds); the five calls the analysis transform makes at the reference width 20 times on two streams; the operand checks.
The only skip in this file is "needs a HIP device"."""
import numpy as np
import pytest
import torch

import sconv_s2_bf16x1_cases as sb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lic():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lic360
    return lic360


def _operands(lic, case, data):
    """the call, its device operands (everything but `out`) and keyword arguments; the weight travels in the STRIDE-1 bf16x1 pack"""
    dev = lambda t: None if t is None else torch.from_numpy(t).cuda()
    conv, pack = (lic.sconv3x3s2_bf16x1, lic.sconv3x3_bf16x1_pack) if case.ks == 3 else (lic.sconv1x1s2_bf16x1, lic.sconv1x1_bf16x1_pack)
    kw = dict(pad=case.pad, oring=case.oring)
    if case.ks == 3:
        kw.update(sphere=bool(case.sphere))
    return conv, (dev(data["x"]), pack(dev(data["w"])), dev(data["b"]), dev(data["slope"]), dev(data["res"])), kw


_REFS = {}                                                                  # production case (xrnd tier) -> float32 reference, shared with the repeatability test


def _reference(case, tier, data):
    key = (case.name, tier)
    if key not in _REFS:
        want64 = sb.reference(case, data)
        want = want64.astype(np.float32)
        assert np.array_equal(want, want64)                                 # the expected values are fp32 numbers
        if not (case.prod and tier == "xrnd"):
            return want
        _REFS[key] = want
    return _REFS[key]


@pytest.mark.parametrize("tier", list(sb.TIERS))
@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: c.name)
def test_sconv_s2_bf16x1_is_exact(lic, case, tier):
    assert (lic.sconv3x3s2_bf16x1_supported if case.ks == 3 else lic.sconv1x1s2_bf16x1_supported)(case.cin, case.cout)
    data = sb.make_case(case, tier)
    bound = sb.assert_exact_domain(case, data)
    want = _reference(case, tier, data)
    conv, ops, kw = _operands(lic, case, data)
    out = torch.full(sb.out_shape(case), sb.SENTINEL, device="cuda:0")
    assert conv(*ops, out, **kw) is out
    got = out.cpu().numpy()
    print("%s / %s: branch %s, |b| + 4 |res| + sum |w~||x~| <= %g" % (case.name, tier, tuple(sb.branch_of(case)), bound))
    assert np.array_equal(got, want), sb.describe_mismatch(case, got, want)


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
    want = torch.from_numpy(_reference(case, "xrnd", data)).cuda()
    conv, ops, kw = _operands(lic, case, data)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty(sb.out_shape(case), device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    try:
        for rep in range(0, 20, 2):
            for k, s in enumerate(streams):
                with torch.cuda.stream(s):
                    outs[k].fill_(sb.SENTINEL)
                    conv(*ops, outs[k], **kw)
            for k, s in enumerate(streams):
                s.synchronize()
                if not torch.equal(outs[k], want):
                    got = outs[k].cpu().numpy()
                    pytest.fail("launch %d (stream %d): %s" % (rep + k, k, sb.describe_mismatch(case, got, want.cpu().numpy())))
    finally:
        torch.cuda.synchronize()


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
        fp32_pack = (lic.sconv3x3_pack if case.ks == 3 else lic.sconv1x1_pack)(torch.from_numpy(data["w"]).cuda())
        with pytest.raises(lic.Lic360Error):
            conv(x, fp32_pack, b, slope, None, None, **kw)                                              # the fp32 stride-2 form's pack
        with pytest.raises(lic.Lic360Error):
            conv(x, packed.float(), b, slope, None, None, **kw)
