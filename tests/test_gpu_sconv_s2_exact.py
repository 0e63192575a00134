"""The stride-2 sphere convolutions (lic360.sconv3x3s2 / sconv1x1s2: the stride-2 forms of the body in csrc/conv3x3_kernels.hip) bit for bit:
integer data on which a convolution has one fp32 result whatever the summation order (tests/sconv_s2_cases.py), so the whole output tensor --
the interior window and the untouched frame in one comparison -- must EQUAL a float64 reference.  The branch matrix on small maps and the five
calls the analysis transform makes at the reference width; every production case 20 times on two streams.
The only skip in this file is "needs a HIP device"."""
import numpy as np
import pytest
import torch

import sconv_s2_cases as s2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lic():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lic360
    return lic360


def _operands(lic, case, data):
    """the call, its device operands (everything but `out`) and keyword arguments; the weight travels in the STRIDE-1 pack"""
    dev = lambda t: None if t is None else torch.from_numpy(t).cuda()
    conv, pack = (lic.sconv3x3s2, lic.sconv3x3_pack) if case.ks == 3 else (lic.sconv1x1s2, lic.sconv1x1_pack)
    kw = dict(pad=case.pad, oring=case.oring)
    if case.ks == 3:
        kw.update(sphere=bool(case.sphere))
    return conv, (dev(data["x"]), pack(dev(data["w"])), dev(data["b"]), dev(data["slope"]), dev(data["res"])), kw


_REFS = {}                                                                  # production case -> float32 reference, shared with the repeatability test


def _reference(case, data):
    if case.name not in _REFS:
        want64 = s2.reference(case, data)
        want = want64.astype(np.float32)
        assert np.array_equal(want, want64)                                 # the expected values are fp32 numbers
        if not case.prod:
            return want
        _REFS[case.name] = want
    return _REFS[case.name]


@pytest.mark.parametrize("case", s2.CASES, ids=lambda c: c.name)
def test_sconv_s2_is_exact(lic, case):
    assert (lic.sconv3x3s2_supported if case.ks == 3 else lic.sconv1x1s2_supported)(case.cin, case.cout)
    data = s2.make_case(case)
    bound = s2.assert_exact_domain(case, data, "fp32")
    want = _reference(case, data)
    conv, ops, kw = _operands(lic, case, data)
    out = torch.full(s2.out_shape(case), s2.SENTINEL, device="cuda:0")
    assert conv(*ops, out, **kw) is out
    got = out.cpu().numpy()
    print("%s: branch %s, |b| + 4 |res| + sum |w||x| <= %g" % (case.name, tuple(s2.branch_of(case)), bound))
    assert np.array_equal(got, want), s2.describe_mismatch(case, got, want)


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
    want = torch.from_numpy(_reference(case, data)).cuda()
    conv, ops, kw = _operands(lic, case, data)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty(s2.out_shape(case), device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    try:
        for rep in range(0, 20, 2):
            for k, s in enumerate(streams):
                with torch.cuda.stream(s):
                    outs[k].fill_(s2.SENTINEL)
                    conv(*ops, outs[k], **kw)
            for k, s in enumerate(streams):
                s.synchronize()
                if not torch.equal(outs[k], want):
                    got = outs[k].cpu().numpy()
                    pytest.fail("launch %d (stream %d): %s" % (rep + k, k, s2.describe_mismatch(case, got, want.cpu().numpy())))
    finally:
        torch.cuda.synchronize()


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
