"""The attention blocks' fused gate (lic360.sconv1x1_gate / _bf16x3 / _bf16x1; kernels k_gate_sconv / k_gate_sconv_b3 / k_gate_sconv_b1) bit for bit: integer
data scaled by a power of two, on which y = conv1x1(x) + bias has one fp32 value whatever the summation order, the project's host / device bit-identical
exponential and correctly rounded fp32 `+`, `/`, `*` (tests/sconv_gate_cases.py) -- so the whole output tensor, window and untouched frame (sentinel 7.0) in
one comparison, must EQUAL the reference.  Every case in every form and tier; the saturation case's special channels; the wrappers' operand refusals; the
production map 10 times on two streams."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_gate_cases as gc
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _fns(lic, form):
    sfx = "" if form == "fp32" else "_" + form
    return getattr(lic, "sconv1x1_gate" + sfx), getattr(lic, "sconv1x1%s_pack" % sfx)


def _operands(lic, case, form, data):
    fn, pack = _fns(lic, form)
    return fn, (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["trunk"]), gs.dev(data["res"])), dict(ring=case.ring, ring_w=case.ring_w)


def _describe(case, form):
    return lambda got, want: gc.describe_mismatch(case, form != "fp32", got, want).replace("bf16x3", form)


@pytest.mark.parametrize("p", gc.PARAMS, ids=gc.ident)
def test_the_gate_is_exact(lic, p):
    case, form, tier = p
    data, want = gc.shared(case, form, tier)
    gc.assert_exact_domain(case, form, tier, data)
    fn, ops, kw = _operands(lic, case, form, data)
    got = gs.sentinel_call(lambda out: fn(*ops, out, **kw), want.shape, gc.SENTINEL)
    print("%s: kernel %s, branch %s" % (gc.ident(p), gc.instantiation(case, form), tuple(gc.branch_of(case, form != "fp32"))))
    gs.check_whole_output(got, want, _describe(case, form))
    if case.name == "g_saturate":
        win = gc.window(case)
        t, r, g = data["trunk"][win], data["res"][win], got[win]
        for bias, chans in gc.SATURATE.items():
            ch = list(chans)
            if bias == 64.0:
                assert np.array_equal(g[:, ch], r[:, ch] + t[:, ch])
            elif bias == -128.0:
                assert np.array_equal(g[:, ch], r[:, ch])
            else:
                assert np.array_equal(g[:, ch], want[win][:, ch]) and not np.array_equal(g[:, ch], r[:, ch])


@pytest.mark.parametrize("form", gc.FORMS)
def test_a_fresh_out_is_zero_filled(lic, form):
    case = gc.BY_NAME["g_q4_low"]
    data, want = gc.shared(case, form, gc.TIERS[form][0])
    fn, ops, kw = _operands(lic, case, form, data)
    got = fn(*ops, **kw).cpu().numpy()
    zeroed = np.zeros_like(want)
    zeroed[gc.window(case)] = want[gc.window(case)]
    assert np.array_equal(got, zeroed)


@pytest.mark.parametrize("form", gc.FORMS)
def test_the_wrappers_refuse_wrong_operands(lic, form):
    case = gc.BY_NAME["g_q4_one"]
    data, _ = gc.shared(case, form, gc.TIERS[form][0])
    fn, (x, pk, b, t, r), kw = _operands(lic, case, form, data)
    out = torch.empty_like(t)
    E = lic.Lic360Error
    with pytest.raises(E):
        fn(x, pk, b, t[:, :, 1:].contiguous(), r, out, **kw)                # wrong shape
    with pytest.raises(E):
        fn(x, pk, b, t, r[:, :96].contiguous(), out, **kw)
    with pytest.raises(E):
        fn(x, pk, b, t, r, out[..., :-1].contiguous(), **kw)
    with pytest.raises(E):
        fn(x, pk, b, t.cpu(), r, out, **kw)                                 # wrong device
    with pytest.raises(E):
        fn(x, pk, b, t, r.cpu(), out, **kw)
    with pytest.raises(E):
        fn(x, pk, b, t.double(), r, out, **kw)                              # wrong dtype
    with pytest.raises(E):
        fn(x, pk, b, t, r.half(), out, **kw)
    with pytest.raises(E):
        fn(x, pk, b, t.transpose(2, 3), r, out, **kw)                       # not contiguous
    with pytest.raises(E):
        fn(x, pk, b, None, r, out, **kw)
    with pytest.raises(E):
        fn(x, pk, b, t, None, out, **kw)
    for other in gc.FORMS:                                                  # another form's pack
        if other != form:
            with pytest.raises(E):
                fn(x, _fns(lic, other)[1](gs.dev(data["w"])), b, t, r, out, **kw)
    with pytest.raises(E):
        fn(x, pk, b, t, r, t, **kw)                                         # out overlapping an input
    with pytest.raises(E):
        fn(x, pk, b, t, r, r, **kw)
    big = torch.empty(2 * t.numel(), device="cuda:0")
    t2, out2 = big[:t.numel()].view(t.shape), big[t.numel() // 2:t.numel() // 2 + t.numel()].view(t.shape)
    with pytest.raises(E):
        fn(x, pk, b, t2, r, out2, **kw)                                     # a partial overlap
    x192 = torch.zeros((1, 192, case.hp, case.wp), device="cuda:0")
    with pytest.raises(E):                                                  # out == x (cin == cout)
        fn(x192, _fns(lic, form)[1](torch.zeros((192, 192, 1, 1), device="cuda:0")), b, t, r, x192, **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", gc.FORMS)
def test_the_production_map_repeats_bit_for_bit(lic, form):
    """10 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the reference"""
    case = gc.BY_NAME["g_prod_132x260"]
    data, want = gc.shared(case, form, gc.TIERS[form][-1])
    fn, ops, kw = _operands(lic, case, form, data)
    gs.repeat_on_two_streams(lambda out: fn(*ops, out, **kw), want.shape, want, gc.SENTINEL, _describe(case, form), launches=10)
