"""The narrow-workgroup sphere convolutions (lic360.sconv3x3_narrow / sconv1x1_narrow / sconv1x1_gate_narrow; kernels k_narrow_conv / k_narrow_gate) bit for bit.
Every case of tests/sconv_narrow_cases.py in every form, tier and cpw on exact integer data: the whole output tensor, window and untouched frame (sentinel 7.0)
in one comparison, must EQUAL the wide forms' float64 reference.  On N(0, 1) data of the same cases the narrow output equals the WIDE kernel's output bit for bit
in every form (an output's sequence of K steps is the same in both).  The production cases 10 times on two streams."""
import numpy as np
import pytest
import torch

import sconv_gate_cases as gc
import sconv_narrow_cases as nc
from gpu_support import check_whole_output, dev as _dev, lic, repeat_on_two_streams, sentinel_call  # noqa: F401

pytestmark = pytest.mark.gpu


def _sfx(form):
    return "" if form == "fp32" else "_" + form


def _conv_call(lic, case, form, data):
    """(narrow(out, cpw), wide(out)) of a case on `data`: the same operands and pack to both"""
    c = case
    name = "sconv%dx%d" % (c.ks, c.ks)
    x, b, slope, res = _dev(data["x"]), _dev(data["b"]), _dev(data["slope"]), _dev(data["res"])
    packed = getattr(lic, name + _sfx(form) + "_pack")(_dev(data["w"]))
    kw = dict(ring=c.ring, ring_w=c.ring_w, crop=c.crop, shuffle=c.shuffle)
    if c.ks == 3:
        kw.update(pad=c.pad, sphere=c.sphere)
    narrow = lambda out, cpw: getattr(lic, name + "_narrow")(x, packed, b, slope, res, out, form=form, cpw=cpw, **kw)
    wide = lambda out: getattr(lic, name + _sfx(form))(x, packed, b, slope, res, out, **kw)
    return narrow, wide


def _gate_call(lic, case, form, data):
    ops = (_dev(data["x"]), getattr(lic, "sconv1x1%s_pack" % _sfx(form))(_dev(data["w"])), _dev(data["b"]), _dev(data["trunk"]), _dev(data["res"]))
    kw = dict(ring=case.ring, ring_w=case.ring_w)
    narrow = lambda out, cpw: lic.sconv1x1_gate_narrow(*ops, out, form=form, cpw=cpw, **kw)
    wide = lambda out: getattr(lic, "sconv1x1_gate" + _sfx(form))(*ops, out, **kw)
    return narrow, wide


@pytest.mark.parametrize("p", nc.params(), ids=nc.ident)
def test_the_narrow_convolutions_are_exact(lic, p):
    n, form, tier, cpw = p
    data, want = nc.shared(n.case, form, tier)
    nc.assert_exact_domain(n.case, form, tier, data)
    narrow, _ = _conv_call(lic, n.case, form, data)
    got = sentinel_call(lambda out: narrow(out, cpw), want.shape, nc.SENTINEL)
    print("%s: branch %s" % (nc.ident(p), tuple(nc.branch_of(n.case, form, cpw))))
    check_whole_output(got, want, lambda g, w: nc.describe_mismatch(n.case, form != "fp32", g, w).replace("bf16x3", form) + " (channel terms are the wide kernel's)")


@pytest.mark.parametrize("p", nc.gate_params(), ids=nc.ident)
def test_the_narrow_gate_is_exact(lic, p):
    case, form, tier, cpw = p
    data, want = gc.shared(case, form, tier)
    gc.assert_exact_domain(case, form, tier, data)
    narrow, _ = _gate_call(lic, case, form, data)
    got = sentinel_call(lambda out: narrow(out, cpw), want.shape, gc.SENTINEL)
    check_whole_output(got, want, lambda g, w: gc.describe_mismatch(case, form != "fp32", g, w).replace("bf16x3", form))


@pytest.mark.parametrize("n", nc.CASES, ids=lambda n: n.case.name)
def test_real_data_gives_the_wide_kernels_bits(lic, n):
    data = nc.real_data(n.case)
    for form in nc.FORMS:
        if not any(nc.supported(form, n.case.ks, n.case.cin, n.case.cout, cpw) for cpw in n.cpws):
            continue
        narrow, wide = _conv_call(lic, n.case, form, data)
        want = wide(torch.full(nc.sc.out_shape(n.case), nc.SENTINEL, device="cuda:0"))
        assert bool(torch.isfinite(want).all()) and bool((want != nc.SENTINEL).any())
        for cpw in n.cpws:
            got = narrow(torch.full_like(want, nc.SENTINEL), cpw)
            assert torch.equal(got, want), (n.case.name, form, cpw, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("case", nc.GATE_CASES, ids=lambda c: c.name)
def test_real_data_gives_the_wide_gates_bits(lic, case):
    data = gc.real_data(case)
    for form in nc.FORMS:
        narrow, wide = _gate_call(lic, case, form, data)
        want = wide(torch.full(data["trunk"].shape, gc.SENTINEL, device="cuda:0"))
        for cpw in nc.CPWS:
            got = narrow(torch.full_like(want, gc.SENTINEL), cpw)
            assert torch.equal(got, want), (case.name, form, cpw, int((got != want).sum()))


@pytest.mark.parametrize("form", nc.FORMS)
def test_a_fresh_out_is_zero_filled_and_wrong_operands_are_refused(lic, form):
    n = nc.BY_NAME["n3_48_low" if form != "fp32" else "n3_q2_cin16"]
    data, want = nc.shared(n.case, form, nc.TIERS[form][0])
    narrow, _ = _conv_call(lic, n.case, form, data)
    got = narrow(None, 48).cpu().numpy()
    c = n.case
    win = (Ellipsis, slice(c.ring, c.hp - c.ring), slice(c.ring_w, c.wp - c.ring_w))      # (neither case crops or shuffles)
    zeroed = np.zeros_like(want)
    zeroed[win] = want[win]
    assert np.array_equal(got, zeroed)
    E = lic.Lic360Error
    with pytest.raises(E):
        narrow(torch.empty((1, c.cout, c.hp, c.wp + 1), device="cuda:0"), 48)
    with pytest.raises(E):
        narrow(None, 96 if c.cout == 96 else 192)                           # not below the pack's block
    with pytest.raises(E):
        narrow(None, 24)
    x = _dev(data["x"])
    with pytest.raises(E):
        lic.sconv3x3_narrow(x, getattr(lic, "sconv3x3%s_pack" % _sfx("bf16x1" if form != "bf16x1" else "bf16x3"))(_dev(data["w"])), _dev(data["b"]), form=form, cpw=48,
                            pad=c.pad, ring=c.ring, ring_w=c.ring_w)          # another form's pack
    with pytest.raises(E):
        lic.sconv3x3_narrow(x, None, _dev(data["b"]), form="fp16", cpw=48)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", nc.PRODUCTION, ids=lambda n: n.case.name)
def test_the_production_layers_repeat_bit_for_bit(lic, n):
    """10 launches per form, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the reference"""
    for form in nc.FORMS:
        cpw = n.cpws[0]
        if not nc.supported(form, n.case.ks, n.case.cin, n.case.cout, cpw):
            continue
        data, want = nc.shared(n.case, form, nc.TIERS[form][-1])
        narrow, _ = _conv_call(lic, n.case, form, data)
        repeat_on_two_streams(lambda out: narrow(out, cpw), want.shape, want, nc.SENTINEL,
                              lambda g, w: "%s: %s" % (form, nc.describe_mismatch(n.case, form != "fp32", g, w)), launches=10)
