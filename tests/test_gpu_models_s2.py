"""The down-sampling layers of the analysis transform on this package's own kernels (lic360.sconv3x3s2 / sconv1x1s2, lic360_models.py):
the two calls against the oracle's pad -> conv2d(stride 2) on random data, ResidualBlockDown and SphereConv2 with stride-2 fusion forced on a small
map against the oracle's blocks (the whole output, aprons included), the switches that send them back to the library (the stride-2 threshold, a
recorded gradient), the bf16x3 mode (stride-2 layers stay fp32), and the analysis transform at the reference width with stride-2 fusion on and off."""
import numpy as np
import pytest
import torch

import gpu_support as gs
from gpu_support import dev, lic  # noqa: F401
from util import _block_params, _refresh

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("case", [(3, 192, 192, 2, 40, 56, True, False), (3, 32, 96, 1, 26, 44, False, True), (3, 16, 192, 3, 12, 20, True, True),
                                  (1, 192, 192, 2, 40, 56, False, True), (1, 32, 96, 1, 26, 44, True, False), (1, 64, 384, 3, 12, 20, True, True)],
                         ids=lambda c: "k%d_%dto%d_n%d_%dx%d" % c[:6])
def test_sconv_s2_matches_the_oracle_conv(lic, case):
    """lic360.sconv3x3s2 / sconv1x1s2 against the oracle's conv2d(sphere_pad_inplace(x), w, b, 2, 3) resp. conv2d(x, w, b, 2, 2) -> PReLU -> + residual
    on the interior window; cells outside the window are not touched"""
    import oracle as orc
    ks, cin, cout, n, hp, wp, act, with_res = case
    rng = np.random.default_rng(7 * cin + cout + wp + ks)
    x = rng.standard_normal((n, cin, hp, wp)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, ks, ks)) * 0.1).astype(np.float32)
    b, sl = rng.standard_normal(cout).astype(np.float32), rng.random(cout).astype(np.float32)
    oh, ow = (hp - 4) // 2, (wp - 4) // 2
    res = rng.standard_normal((n, cout, oh + 4, ow + 4)).astype(np.float32) if with_res else None
    want = orc.conv2d(orc.sphere_pad_inplace(x.copy(), 2), w, b, 2, 3) if ks == 3 else orc.conv2d(x, w, b, 2, 2)
    assert want.shape == (n, cout, oh + 4, ow + 4)
    if act:
        want = orc.prelu(want, sl)
    if with_res:
        want = want + res
    out = torch.full((n, cout, oh + 4, ow + 4), 7.0, device="cuda:0")
    if ks == 3:
        lic.sconv3x3s2(dev(x), lic.sconv3x3_pack(dev(w)), dev(b), dev(sl) if act else None, dev(res), out, pad=2, sphere=True, oring=2)
    else:
        lic.sconv1x1s2(dev(x), lic.sconv1x1_pack(dev(w)), dev(b), dev(sl) if act else None, dev(res), out, pad=2, oring=2)
    got = out.cpu().numpy()
    win = (slice(None), slice(None), slice(2, 2 + oh), slice(2, 2 + ow))
    assert np.allclose(got[win], want[win], rtol=1e-4, atol=1e-4), float(np.abs(got[win] - want[win]).max())
    frame = np.ones(got.shape, bool)
    frame[win] = False
    assert np.all(got[frame] == 7.0)


def _blocks(lm, c):
    """(module, oracle function of (x, params)) of the two down-sampling modules at c channels, 1-d / 2-d parameters moved off their initial values"""
    import oracle as orc

    def sphere_conv2(x, p):                                                # model_zoo.py:96-106: pad -> conv -> trim
        return orc.sphere_trim(orc.conv2d(orc.sphere_pad_inplace(x.copy(), 2), p["conv.weight"], p["conv.bias"], 2, 3), 2)
    out = []
    for blk, fn in ((lm.ResidualBlockDown(c, c, 0), orc.blocks.residual_down), (lm.SphereConv2(c, c, 3, 2, 3, 0), sphere_conv2)):
        out.append((gs.jitter(blk.to("cuda:0")), fn))
    return out


def test_down_blocks_fused_match_the_oracle_at_full_width(lic, monkeypatch):
    """ResidualBlockDown(192, 192) and SphereConv2(192, 192, 3, 2, 3) with fusion forced on a small map against the oracle's blocks, the whole
    output, aprons included; the launches are counted.  Then the same modules with stride-2 fusion alone switched off: no stride-2 call, the same
    result; and with every fused threshold out of reach: the whole block on the library."""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    torch.manual_seed(16)
    c = 192
    x = _refresh(torch.randn((2, c, 44, 76), device="cuda:0")).contiguous()   # interior 40 x 72 -> 20 x 36: ragged in rows and columns
    xn = x.cpu().numpy()
    rec = gs.SconvCalls(lic, monkeypatch)
    calls = rec.counts
    expect = {"ResidualBlockDown": dict(sconv3x3s2=1, sconv1x1s2=1, sconv3x3=1), "SphereConv2": dict(sconv3x3s2=1)}
    with torch.no_grad():
        for blk, fn in _blocks(lm, c):
            name = type(blk).__name__
            rec.reset()
            xin = x.clone()
            got = blk(xin)
            assert rec.only(**expect[name]), (name, rec.made())
            assert torch.equal(xin, x), name + ": the fused path must not modify its input"
            got = got.cpu().numpy()
            want = fn(xn.copy(), _block_params(blk))
            assert got.shape == want.shape == (2, c, 24, 40)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-4), "%s: max abs error %g" % (name, np.abs(got - want).max())
            assert not got[:, :, :2].any() and not got[:, :, -2:].any() and not got[:, :, :, :2].any() and not got[:, :, :, -2:].any()
            # stride-2 fusion alone off
            monkeypatch.setattr(lm, "FUSED_S2_MIN_WORKGROUPS", 1 << 30)
            rec.reset()
            lib = blk(x.clone()).cpu().numpy()
            assert calls["sconv3x3s2"] == 0 and calls["sconv1x1s2"] == 0, (name, calls)
            assert calls["sconv3x3"] == (1 if name == "ResidualBlockDown" else 0), (name, calls)     # the stride-1 conv2 stays fused
            assert np.allclose(lib, got, rtol=1e-4, atol=1e-4) and np.allclose(lib, want, rtol=1e-4, atol=1e-4), name
            monkeypatch.setattr(lm, "FUSED_S2_MIN_WORKGROUPS", 0)
        # the stride-1 threshold out of reach: the whole Down block goes down the library path
        blk = _blocks(lm, c)[0][0]
        monkeypatch.setattr(lm, "FUSED_MIN_WORKGROUPS", 1 << 30)
        rec.reset()
        lib = blk(x.clone())
        assert not rec.made(), rec.made()
        gs.count_rule(monkeypatch, lm)
        assert torch.allclose(blk(x.clone()), lib, rtol=1e-4, atol=1e-4)


def test_a_recorded_gradient_keeps_the_library_sequence(lic, monkeypatch):
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    torch.manual_seed(17)
    c = 192
    x = _refresh(torch.randn((1, c, 20, 36), device="cuda:0")).contiguous()
    rec = gs.SconvCalls(lic, monkeypatch)
    calls = rec.counts
    for blk, _ in _blocks(lm, c):
        name = type(blk).__name__
        assert all(p.requires_grad for p in blk.parameters())
        rec.reset()
        y = blk(x.clone())
        assert not rec.made(), (name, rec.made())
        y.square().mean().backward()
        for pname, p in blk.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (name, pname)
        conv = blk.conv1 if name == "ResidualBlockDown" else blk.conv
        assert float(conv.weight.grad.abs().max()) > 0, name
        with torch.no_grad():                                               # and without recording the same module goes fused
            rec.reset()
            y2 = blk(x.clone())
            assert calls["sconv3x3s2"] == 1, (name, calls)
            assert torch.allclose(y2, y.detach(), rtol=1e-4, atol=1e-4), name
        for p in blk.parameters():                                          # one parameter with requires_grad is enough
            p.requires_grad_(False)
        next(iter(blk.parameters())).requires_grad_(True)
        rec.reset()
        blk(x.clone())
        assert calls["sconv3x3s2"] == 0 and calls["sconv1x1s2"] == 0, (name, calls)


def test_bf16x3_mode_keeps_the_stride_2_layers_on_fp32(lic, monkeypatch):
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    torch.manual_seed(18)
    c = 192
    x = _refresh(torch.randn((1, c, 20, 36), device="cuda:0")).contiguous()
    rec = gs.SconvCalls(lic, monkeypatch)
    calls = rec.counts
    with torch.no_grad():
        (down, fn), (sc2, _) = _blocks(lm, c)
        want = down(x.clone())
        lm.set_conv_precision(down, "bf16x3")
        lm.set_conv_precision(sc2, "bf16x3")
        rec.reset()
        got = down(x.clone())
        assert rec.only(sconv3x3s2=1, sconv1x1s2=1, sconv3x3_bf16x3=1), rec.made()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4)
        rec.reset()
        sc2(x.clone())
        assert rec.only(sconv3x3s2=1), rec.made()


def test_analysis_transform_with_and_without_stride_2_fusion(lic, monkeypatch):
    """EncoderV2 at 192 channels, batch 8, 512 x 1024, seeded: the outputs of the two hidden down-sampling stages and of SphereConv2 with stride-2
    fusion on and off (stride-1 fusion on in both runs) agree within 1e-4 of the stage's own range -- the bound
    test_whole_codec_in_bf16x3_mode_at_the_reference_width uses between two arithmetic orders of these networks."""
    import lic360_models as lm
    rec = gs.SconvCalls(lic, monkeypatch)
    calls = rec.counts
    torch.manual_seed(19)
    enc = lm.EncoderV2(192, 192, 0).to("cuda:0").eval()
    stages, seen = (2, 5, 7), {}
    with torch.no_grad():
        img = torch.rand((8, 3, 512, 1024), device="cuda:0")
        mode = ["fused"]
        hooks = [enc.net[i].register_forward_hook(lambda m, a, o, i=i: seen.setdefault((mode[0], i), o.clone())) for i in stages]
        rec.reset()
        code, imp = enc(img)
        fused_calls = dict(calls)
        assert calls["sconv3x3s2"] >= 1 and calls["sconv3x3"] >= 1, calls
        monkeypatch.setattr(lm, "FUSED_S2_MIN_WORKGROUPS", 1 << 30)
        mode[0] = "library"
        rec.reset()
        code_l, imp_l = enc(img)
        assert calls["sconv3x3s2"] == 0 and calls["sconv1x1s2"] == 0 and calls["sconv3x3"] >= 1, calls
        for h in hooks:
            h.remove()
    print("stride-2 calls with fusion on: %s" % fused_calls)
    for i in stages:
        a, b = seen[("fused", i)], seen[("library", i)]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        di, si = float((a - b).abs().max()), float(b.abs().max())
        print("analysis stage %d: max |s2 fused - library| = %g, max |library| = %g" % (i, di, si))
        assert di <= 1e-4 * si, (i, di, si)
    assert bool(torch.isfinite(code).all()) and bool(torch.isfinite(imp).all())
    print("code: max |fused - library| = %g; importance map: %g" % (float((code - code_l).abs().max()), float((imp - imp_l).abs().max())))
