"""The stride-2 sphere convolutions (lic360.sconv3x3s2 / sconv1x1s2: the stride-2 forms of the body in csrc/conv3x3_kernels.hip) bit for bit:
integer data on which a convolution has one fp32 result whatever the summation order (tests/sconv_s2_cases.py), so the whole output tensor --
the interior window and the untouched frame in one comparison -- must EQUAL a float64 reference.  The branch matrix on small maps and the five
calls the analysis transform makes at the reference width; every production case 20 times on two streams.
There is no skip in this file: without a HIP device its tests fail."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_s2_cases as s2
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _operands(lic, case, data):
    """the call, its device operands (everything but `out`) and keyword arguments; the weight travels in the STRIDE-1 pack"""
    conv, pack = (lic.sconv3x3s2, lic.sconv3x3_pack) if case.ks == 3 else (lic.sconv1x1s2, lic.sconv1x1_pack)
    kw = dict(pad=case.pad, oring=case.oring)
    if case.ks == 3:
        kw.update(sphere=bool(case.sphere))
    return conv, (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"])), kw


def _call(lic, case, data):
    conv, ops, kw = _operands(lic, case, data)
    return lambda out: conv(*ops, out, **kw)


def _reference(case, data):
    """a production case's reference is kept: shared with the repeatability test"""
    return gs.fp32_reference(lambda: s2.reference(case, data), ("sconv_s2", case.name) if case.prod else None)


@pytest.mark.parametrize("case", s2.CASES, ids=lambda c: c.name)
def test_sconv_s2_is_exact(lic, case):
    assert (lic.sconv3x3s2_supported if case.ks == 3 else lic.sconv1x1s2_supported)(case.cin, case.cout)
    data = s2.make_case(case)
    bound = s2.assert_exact_domain(case, data, "fp32")
    want = _reference(case, data)
    got = gs.sentinel_call(_call(lic, case, data), s2.out_shape(case), s2.SENTINEL)
    print("%s: branch %s, |b| + 4 |res| + sum |w||x| <= %g" % (case.name, tuple(s2.branch_of(case)), bound))
    gs.check_whole_output(got, want, lambda g, w: s2.describe_mismatch(case, g, w))


def test_a_fresh_out_is_zero_filled(lic):
    """without `out`: the interior window in a map of zeros (SphereTrim applied)"""
    case = next(c for c in s2.SMALL if c.name == "d3_q4_one_tile")
    data = s2.make_case(case)
    assert case.oring == 2
    frame = np.ones(s2.out_shape(case), bool)
    frame[:, :, 2:-2, 2:-2] = False
    want = np.where(frame, np.float32(0), _reference(case, data))
    conv, ops, kw = _operands(lic, case, data)
    got = conv(*ops, **kw).cpu().numpy()
    assert np.array_equal(got, want), s2.describe_mismatch(case, got, want)


@pytest.mark.parametrize("case", s2.PRODUCTION, ids=lambda c: c.name)
def test_production_cases_repeat_bit_for_bit(lic, case):
    """20 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the
    reference.  Determinism under ordinary use (two streams, ordinary arguments); stops at the first difference."""
    data = s2.make_case(case)
    gs.repeat_on_two_streams(_call(lic, case, data), s2.out_shape(case), _reference(case, data), s2.SENTINEL, lambda g, w: s2.describe_mismatch(case, g, w))


def test_operand_checks_refuse_before_the_kernel(lic):
    """the package's operand checks on the down-sampled shapes: a wrong `out` or `residual` is an error, not an out-of-bounds device access"""
    case = next(c for c in s2.SMALL if c.name == "d3_q4_one_tile")
    data = s2.make_case(case)
    conv, ops, kw = _operands(lic, case, data)
    x, packed, b, slope, _ = ops
    with pytest.raises(lic.Lic360Error):
        conv(x, packed, b, slope, None, torch.empty((1, 192, 36, 36), device="cuda:0"), **kw)         # the input's shape, not the output's
    with pytest.raises(lic.Lic360Error):
        conv(x, packed, b, slope, torch.empty((1, 192, 36, 36), device="cuda:0"), None, **kw)
    with pytest.raises(lic.Lic360Error):
        conv(x[:, :, :-1].contiguous(), packed, b, slope, None, None, **kw)                             # an odd interior
    with pytest.raises(lic.Lic360Error):
        conv(x, packed[:-4], b, slope, None, None, **kw)
    with pytest.raises(lic.Lic360Error):
        conv(x, packed.double(), b, slope, None, None, **kw)
