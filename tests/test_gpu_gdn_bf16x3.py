"""The split-bf16 one-pass GDN (csrc/gdn_bf16x3.inc) on real-valued data, and its way up to the models: single calls held to the stated bound -- 2^-15
relative per element against the float64 GDN of the same fp32 operands, for gamma >= 0 (tests/gdn_bf16x3_cases.py: the bound passes the split form and fails
a form without lo parts) -- then lic360_operator.GDN in "bf16x3" mode, the two blocks that hold a GDN under set_conv_precision(.., gdn="bf16x3"), and the way
back to fp32."""
import numpy as np
import pytest
import torch

import gdn_bf16x3_cases as gc
import gpu_support as gs
from gpu_support import dev, lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _seeded_gdn(c, inverse, seed=0):
    """a lic360_operator.GDN whose raw parameters give a dense non-negative effective gamma (gdn_bf16x3_cases.real_params)"""
    import lic360_operator as lo
    m = lo.GDN(c, 0, inverse).to("cuda:0")
    g, b = gc.real_params(c, seed)
    with torch.no_grad():
        m.gamma.copy_(dev(g))
        m.beta.copy_(dev(b))
    return m


def _effective(m):
    """the module's own reparametrisation (extras.py: GDN.forward), as float32 numpy"""
    with torch.no_grad():
        beta = m.beta.clamp_min(m.beta_bound) ** 2 - m.pedestal
        gamma = m.gamma.clamp_min(m.gamma_bound) ** 2 - m.pedestal
    return gamma.cpu().numpy(), beta.cpu().numpy()


def _held_to_the_bound(what, got, x, gamma, beta, inverse):
    err = gc.max_rel_err(got.cpu().numpy(), gc.gdn_float64(x.cpu().numpy(), gamma, beta, inverse))
    print("%s: max relative error %.3g (bound %.3g)" % (what, err, gc.BOUND))
    assert err < gc.BOUND, "%s: max relative error %g against the float64 GDN, bound %g" % (what, err, gc.BOUND)
    return err


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0])
@pytest.mark.parametrize("c", [96, 192])
def test_single_calls_are_held_to_the_bound(lic, c, scale, inverse):
    m = _seeded_gdn(c, inverse)
    gamma, beta = _effective(m)
    assert np.allclose(gamma, gc.effective(*gc.real_params(c, 0))[0], rtol=1e-6, atol=0) and gamma.min() >= 0 and beta.min() > 0   # the data of the CPU test
    x = dev(gc.real_x(c, scale))
    g, b = dev(gamma), dev(beta)
    got = lic.gdn_bf16x3_forward(x, lic.gdn_bf16x3_pack(g), b, inverse)
    _held_to_the_bound("c %d, scale %g, inverse %s" % (c, scale, inverse), got, x, gamma, beta, inverse)
    fp32 = lic.gdn_forward(x, g, b, inverse)                                # and it is not the fp32 kernel under another name
    assert not torch.equal(got, fp32)


def _recording(lic, monkeypatch):
    """wrap both GDN entry points and the pack: names in call order, and the new form's (x, beta, inverse, out) per call"""
    seen = {"names": [], "b3": [], "packs": 0}
    real_f, real_b3, real_pack = lic.gdn_forward, lic.gdn_bf16x3_forward, lic.gdn_bf16x3_pack

    def fwd(x, *a, **k):
        seen["names"].append("fp32")
        return real_f(x, *a, **k)

    def b3(x, packed, beta, inverse=False, out=None):
        seen["names"].append("bf16x3")
        xin = x.clone()
        y = real_b3(x, packed, beta, inverse, out)
        seen["b3"].append((xin, beta.clone(), bool(inverse), y.clone()))
        return y

    def pack(gamma):
        seen["packs"] += 1
        return real_pack(gamma)
    monkeypatch.setattr(lic, "gdn_forward", fwd)
    monkeypatch.setattr(lic, "gdn_bf16x3_forward", b3)
    monkeypatch.setattr(lic, "gdn_bf16x3_pack", pack)
    return seen


def test_the_module_reaches_the_kernel_and_repacks(lic, monkeypatch):
    """lic360_operator.GDN in "bf16x3" mode calls gdn_bf16x3_forward with the whole padded map, packs once per written gamma, and is held to the bound"""
    import lic360_models as lm
    seen = _recording(lic, monkeypatch)
    m = _seeded_gdn(192, True)
    torch.manual_seed(3)
    x = torch.randn((1, 192, 68, 132), device="cuda:0")
    with torch.no_grad():
        want32 = m(x)
        assert seen["names"] == ["fp32"] and seen["packs"] == 0             # the default is the fp32 kernel
        assert lm.set_conv_precision(m, "fp32", gdn="bf16x3") is m and m._gdn_precision == "bf16x3"
        y = m(x)
        assert seen["names"] == ["fp32", "bf16x3"] and seen["packs"] == 1
        assert tuple(seen["b3"][0][0].shape) == (1, 192, 68, 132) and tuple(y.shape) == (1, 192, 68, 132) and seen["b3"][0][2] is True
        _held_to_the_bound("module, 68x132", y, x, *_effective(m), True)
        assert not torch.equal(y, want32)
        assert torch.equal(m(x), y) and seen["packs"] == 1                  # the pack is cached
        m.gamma.mul_(1.25)                                                   # an in-place write: the version counter moves, the pointer does not
        y2 = m(x)
        assert seen["packs"] == 2 and not torch.equal(y2, y)
        _held_to_the_bound("module, rewritten gamma", y2, x, *_effective(m), True)
        lm.set_conv_precision(m, "fp32")                                     # without the keyword: back to fp32
        n = len(seen["names"])
        m(x)
        assert seen["names"][n:] == ["fp32"]


@pytest.mark.parametrize("c", [48, 16])
def test_unsupported_channel_counts_stay_on_the_fp32_kernel(lic, monkeypatch, c):
    seen = _recording(lic, monkeypatch)
    m = _seeded_gdn(c, False)
    torch.manual_seed(4)
    x = torch.randn((2, c, 9, 14), device="cuda:0")
    with torch.no_grad():
        want = m(x)
        m._gdn_precision = "bf16x3"
        got = m(x)
    assert seen["names"] == ["fp32", "fp32"] and seen["packs"] == 0
    assert torch.equal(got, want)


def test_a_recorded_gradient_takes_the_torch_path(lic, monkeypatch):
    seen = _recording(lic, monkeypatch)
    m = _seeded_gdn(96, False)
    m._gdn_precision = "bf16x3"
    torch.manual_seed(5)
    x = torch.randn((1, 96, 6, 10), device="cuda:0")
    y = m(x)                                                                 # the parameters require a gradient and recording is on
    assert seen["names"] == [] and y.requires_grad
    y.sum().backward()
    assert m.gamma.grad is not None and bool(torch.isfinite(m.gamma.grad).all())
    with torch.no_grad():
        y3 = m(x)
    assert seen["names"] == ["bf16x3"]
    assert torch.allclose(y3, y.detach(), rtol=1e-4, atol=0)


@pytest.mark.parametrize("which", ["down", "up"])
def test_blocks_with_a_gdn(lic, monkeypatch, which):
    """ResidualBlockDown(192, 192) / ResidualBlockUp(192) at batch 2 on maps that pass _fusable, under set_conv_precision(m, "fp32", gdn="bf16x3"): one GDN
    call per forward, on the new form, held to the single-call bound on its own input; the convolutions are the fp32 run's; and fp32 -> bf16x3 -> fp32
    returns the fp32 bits"""
    import lic360_models as lm
    from util import _refresh
    torch.manual_seed(11)
    c = 192
    if which == "down":
        blk, shape = lm.ResidualBlockDown(c, c, 0).to("cuda:0").eval(), (2, c, 260, 516)
    else:
        blk, shape = lm.ResidualBlockUp(c, 0).to("cuda:0").eval(), (2, c, 68, 132)
    g, b = gc.real_params(c, 1)
    with torch.no_grad():
        blk.relu2.gamma.copy_(dev(g))
        blk.relu2.beta.copy_(dev(b))
    x = _refresh(torch.randn(shape, device="cuda:0")).contiguous()
    seen, calls = _recording(lic, monkeypatch), gs.SconvCalls(lic, monkeypatch)
    with torch.no_grad():
        want32 = blk(x.clone())
        calls32 = calls.made()
        assert seen["names"] == ["fp32"] and sum(calls32.values()) == 3 and all("bf16" not in k for k, v in calls32.items() if v), calls32
        lm.set_conv_precision(blk, "fp32", gdn="bf16x3")
        calls.reset()
        got = blk(x.clone())
        assert seen["names"] == ["fp32", "bf16x3"] and seen["packs"] == 1
        assert calls.made() == calls32, (calls.made(), calls32)
        xin, beta, inverse, y = seen["b3"][0]
        assert tuple(xin.shape) == (2, c, 132, 260) and inverse == (which == "up")
        gamma_e, beta_e = _effective(blk.relu2)
        assert np.array_equal(beta.cpu().numpy(), beta_e)
        win = (Ellipsis, slice(2, -2), slice(2, -2))                        # (the frame of conv2's output is uninitialised scratch, trimmed behind the GDN)
        _held_to_the_bound("block %s" % which, y[win], xin[win], gamma_e, beta_e, inverse)
        assert not torch.equal(got, want32) and torch.allclose(got, want32, rtol=1e-3, atol=1e-3)
        lm.set_conv_precision(blk, "fp32")
        assert torch.equal(blk(x.clone()), want32)
        assert seen["names"] == ["fp32", "bf16x3", "fp32"]
