"""The split-bf16 ("bf16x3") form of the transforms' sphere convolutions (csrc/sconv_bf16x3.inc, lic360.sconv3x3_bf16x3 / sconv1x1_bf16x3,
lic360_models.set_conv_precision): the kernels against the oracle's restatement of what they replace, with a bound that proves the lo terms
are computed (16x below single-pass bf16); the blocks at the reference width; the default path unchanged; the whole codec in bf16x3 mode."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_support as gs
from gpu_support import dev, lic  # noqa: F401
from util import _block_params, _refresh

pytestmark = pytest.mark.gpu


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def _conv_bf16(x, w, b, pad):
    """single-pass bf16 on the CPU: x and w rounded to bf16, the convolution in float64"""
    xd, wd = torch.from_numpy(_bf16(x)).double(), torch.from_numpy(_bf16(w)).double()
    return F.conv2d(xd, wd, torch.from_numpy(b).double(), 1, pad).numpy()


def _check(got, want, want_bf16, win):
    err = float(np.abs(got[win] - want[win]).max())
    err16 = float(np.abs(want_bf16[win] - want[win]).max())
    assert np.allclose(got[win], want[win], rtol=1e-4, atol=1e-4), err
    assert 16 * err <= err16, "bf16x3 error %g is not 16x below single-pass bf16's %g" % (err, err16)
    frame = np.ones(got.shape, bool)
    frame[win] = False
    assert np.all(got[frame] == 7.0)


# (cin, cout, hp, wp, ring, sphere, crop, act, residual, ring_w): the cases of test_gpu_models.py::test_sconv3x3_matches_the_oracle_conv this form
# takes (cin % 32 == 0), the transforms' 192 -> 192 / 96 -> 96 layers with ResidualBlockV2's windows, tall last tile rows (16 k + 2 rows at 192, 16 k + 3 at 96)
CASES3 = [(32, 96, 20, 36, 2, 1, 0, True, True, 2), (32, 384, 18, 34, 2, 0, 0, False, True, 2), (64, 96, 9, 70, 1, 1, 0, False, False, 1),
          (32, 192, 22, 40, 1, 1, 0, True, False, 2), (192, 192, 21, 37, 1, 2, 0, True, True, 2), (192, 192, 38, 24, 2, 1, 0, True, False, 2),
          (96, 96, 23, 40, 2, 1, 0, True, True, 2), (192, 192, 20, 36, 1, 1, 0, True, False, 2)]


@pytest.mark.parametrize("case", CASES3, ids=lambda c: "%dto%d_%dx%d_ring%d_%d_sphere%d" % (c[0], c[1], c[2], c[3], c[4], c[9], c[5]))
def test_sconv3x3_bf16x3_matches_the_oracle_conv(lic, case):
    import oracle as orc
    cin, cout, hp, wp, ring, sphere, crop, act, with_res, ring_w = case
    assert lic.sconv3x3_bf16x3_supported(cin, cout)
    rng = np.random.default_rng(cin + 7 * cout + hp)
    x = rng.standard_normal((2, cin, hp, wp)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.1).astype(np.float32)
    b, sl = rng.standard_normal(cout).astype(np.float32), rng.random(cout).astype(np.float32)
    res = rng.standard_normal((2, cout, hp, wp)).astype(np.float32) if with_res else None
    xin = x
    if sphere == 1:
        xin = orc.sphere_pad_inplace(x.copy(), 2)
    elif sphere == 2:
        xin = x.copy()
        xin[..., :2], xin[..., wp - 2:] = x[..., wp - 4:wp - 2], x[..., 2:4]
    want, want16 = orc.conv2d(xin, w, b, 1, 1 - crop), _conv_bf16(xin, w, b, 1 - crop)
    if act:
        want, want16 = orc.prelu(want, sl), np.where(want16 > 0, want16, want16 * sl[None, :, None, None])
    if with_res:
        want, want16 = want + res, want16 + res
    out = torch.full((2, cout, hp - 2 * crop, wp - 2 * crop), 7.0, device="cuda:0")
    lic.sconv3x3_bf16x3(dev(x), lic.sconv3x3_bf16x3_pack(dev(w)), dev(b), dev(sl) if act else None, dev(res), out, pad=2, sphere=sphere, ring=ring,
                        crop=crop, ring_w=ring_w)
    win = (slice(None), slice(None), slice(ring - crop, hp - crop - ring), slice(ring_w - crop, wp - crop - ring_w))
    _check(out.cpu().numpy(), want, want16, win)


def test_sconv3x3_bf16x3_fuses_the_pixel_shuffle(lic):
    """ResidualBlockUp.conv1 at the reference width: 192 -> 768, unpadded (crop = 1), PReLU, stored through Dtow(2)"""
    import oracle as orc
    cin, cout, hp, wp = 192, 768, 14, 22
    rng = np.random.default_rng(78)
    x = rng.standard_normal((2, cin, hp, wp)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    b, sl = rng.standard_normal(cout).astype(np.float32), rng.random(cout).astype(np.float32)
    xp = orc.sphere_pad_inplace(x.copy(), 2)
    want = orc.dtow(orc.prelu(orc.conv2d(xp, w, b, 1, 0), sl), 2, True)
    c16 = _conv_bf16(xp, w, b, 0)
    want16 = orc.dtow(np.where(c16 > 0, c16, c16 * sl[None, :, None, None]).astype(np.float32), 2, True)
    out = torch.full((2, cout // 4, 2 * (hp - 2), 2 * (wp - 2)), 7.0, device="cuda:0")
    lic.sconv3x3_bf16x3(dev(x), lic.sconv3x3_bf16x3_pack(dev(w)), dev(b), dev(sl), None, out, pad=2, sphere=1, ring=2, crop=1, shuffle=True)
    got = out.cpu().numpy()
    assert got.shape == want.shape
    _check(got, want, want16, (slice(None), slice(None), slice(2, 2 * (hp - 2) - 2), slice(2, 2 * (wp - 2) - 2)))


@pytest.mark.parametrize("case", [(192, 96, 20, 36, 2, 2, True, False), (96, 192, 21, 37, 2, 2, False, True), (64, 384, 12, 20, 1, 3, True, True)],
                         ids=lambda c: "%dto%d_%dx%d" % (c[0], c[1], c[2], c[3]))
def test_sconv1x1_bf16x3_matches_the_oracle_conv(lic, case):
    import oracle as orc
    cin, cout, hp, wp, ring, ring_w, act, with_res = case
    rng = np.random.default_rng(3 * cin + cout + wp)
    x = rng.standard_normal((2, cin, hp, wp)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 1, 1)) * 0.1).astype(np.float32)
    b, sl = rng.standard_normal(cout).astype(np.float32), rng.random(cout).astype(np.float32)
    res = rng.standard_normal((2, cout, hp, wp)).astype(np.float32) if with_res else None
    want, want16 = orc.conv2d(x, w, b, 1, 0), _conv_bf16(x, w, b, 0)
    if act:
        want, want16 = orc.prelu(want, sl), np.where(want16 > 0, want16, want16 * sl[None, :, None, None])
    if with_res:
        want, want16 = want + res, want16 + res
    out = torch.full((2, cout, hp, wp), 7.0, device="cuda:0")
    lic.sconv1x1_bf16x3(dev(x), lic.sconv1x1_bf16x3_pack(dev(w)), dev(b), dev(sl) if act else None, dev(res), out, ring=ring, ring_w=ring_w)
    _check(out.cpu().numpy(), want, want16, (slice(None), slice(None), slice(ring, hp - ring), slice(ring_w, wp - ring_w)))


def test_sconv1x1_bf16x3_shuffled_shortcut(lic):
    """ResidualBlockUp's shortcut at the reference width: cut_edge(1) -> 1x1 192 -> 768 -> Dtow(2), + the (shuffled) residual, one launch"""
    import oracle as orc
    cin, cout, hp, wp = 192, 768, 14, 22
    rng = np.random.default_rng(79)
    x = rng.standard_normal((2, cin, hp, wp)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 1, 1)) * 0.1).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((2, cout // 4, 2 * (hp - 2), 2 * (wp - 2))).astype(np.float32)
    xc = np.ascontiguousarray(x[..., 1:-1, 1:-1])
    want = orc.dtow(orc.conv2d(xc, w, b, 1, 0), 2, True) + res
    want16 = orc.dtow(_conv_bf16(xc, w, b, 0).astype(np.float32), 2, True) + res
    out = torch.full(res.shape, 7.0, device="cuda:0")
    lic.sconv1x1_bf16x3(dev(x), lic.sconv1x1_bf16x3_pack(dev(w)), dev(b), None, dev(res), out, ring=2, crop=1, shuffle=True)
    _check(out.cpu().numpy(), want, want16, (slice(None), slice(None), slice(2, 2 * (hp - 2) - 2), slice(2, 2 * (wp - 2) - 2)))


def test_pack_layout_and_operand_checks(lic):
    """the packed stream is the documented layout ([blk][it = (cg ks + kw) ks + kh][mq][mt][hl][lane] x 8 bf16, csrc/sconv_bf16x3.inc), hi + lo of
    each weight; an fp32 pack is refused by the bf16x3 call and a bf16x3 pack by the fp32 call"""
    rng = np.random.default_rng(80)
    for ks, cin, cout in ((3, 64, 192), (1, 96, 96)):
        w = rng.standard_normal((cout, cin, ks, ks)).astype(np.float32)
        pk = (lic.sconv3x3_bf16x3_pack if ks == 3 else lic.sconv1x1_bf16x3_pack)(torch.from_numpy(w).cuda())
        nq = 4 if cout % 192 == 0 else 2
        got = pk.float().cpu().numpy().reshape(cout // (48 * nq), cin // 32 * ks * ks, nq, 3, 2, 4, 16, 8)   # [blk][it][mq][mt][hl][kq][i][j]
        ref = np.empty(got[:, :, :, :, 0].shape, np.float32)                                              # [blk][it][mq][mt][kq][i][j]
        for blk, it, mq, mt, kq, i in np.ndindex(*ref.shape[:6]):
            kh, kw, cg = it % ks, it // ks % ks, it // (ks * ks)
            ref[blk, it, mq, mt, kq, i] = w[blk * nq * 48 + 48 * mq + 16 * mt + i, 32 * cg + 8 * kq + np.arange(8), kh, kw]
        hi, lo = got[:, :, :, :, 0], got[:, :, :, :, 1]
        assert np.array_equal(hi, _bf16(ref)), "hi planes"
        assert np.array_equal(lo, _bf16(ref - hi)), "lo planes"
    x = torch.zeros((1, 64, 20, 36), device="cuda:0")
    w = torch.from_numpy(rng.standard_normal((192, 64, 3, 3)).astype(np.float32)).cuda()
    b = torch.zeros(192, device="cuda:0")
    with pytest.raises(lic.Lic360Error):
        lic.sconv3x3_bf16x3(x, lic.sconv3x3_pack(w), b, ring=2)
    with pytest.raises(lic.Lic360Error):
        lic.sconv3x3(x, lic.sconv3x3_bf16x3_pack(w), b, ring=2)
    assert not lic.sconv3x3_bf16x3_supported(16, 192) and not lic.sconv1x1_bf16x3_supported(48, 96)
    # the launch's argument contract, both precisions: each of these is refused by the native check ("bad argument") before anything is launched
    cin, cout, hp, wp = 64, 192, 20, 36
    x = torch.zeros((1, cin, hp, wp), device="cuda:0")
    b, sl = torch.zeros(cout, device="cuda:0"), torch.ones(cout, device="cuda:0")
    off = lambda t: torch.cat([t[:1], t])[1:]                               # the same values 4 bytes past a 16-byte boundary
    for ks in (3, 1):
        for form in ("", "_bf16x3"):
            conv, pack = getattr(lic, "sconv%dx%d%s" % (ks, ks, form)), getattr(lic, "sconv%dx%d%s_pack" % (ks, ks, form))
            w = torch.from_numpy(rng.standard_normal((cout, cin, ks, ks)).astype(np.float32)).cuda()
            pk, kw = pack(w), (dict(pad=2, sphere=1) if ks == 3 else {})
            for ci, co in ((40, 192), (64, 100), (8, 96), (64, 48)):        # unsupported channel counts
                with pytest.raises(lic.Lic360Error, match="not supported" if form else "bad argument"):
                    pack(torch.zeros((co, ci, ks, ks), device="cuda:0"))
            crop1 = (1, cout, hp - 2, wp - 2)
            for what, shape, args, kws in (
                    ("ring below ks / 2", (1, cout, hp, wp), (x, pk, b, sl, None), dict(ring=ks // 2 - 1)),
                    ("crop above ring", (1, cout, hp - 6, wp - 6), (x, pk, b, sl, None), dict(ring=2, crop=3)),
                    ("residual with crop and no shuffle", crop1, (x, pk, b, sl, torch.zeros(crop1, device="cuda:0")), dict(ring=2, crop=1)),
                    ("misaligned bias", (1, cout, hp, wp), (x, pk, off(b), sl, None), dict(ring=2)),
                    ("misaligned slope", (1, cout, hp, wp), (x, pk, b, off(sl), None), dict(ring=2))):
                out = torch.full(shape, 777.0, device="cuda:0")
                with pytest.raises(lic.Lic360Error, match="bad argument"):
                    conv(*args, out, **kws, **kw)
                torch.cuda.synchronize()
                assert bool((out == 777.0).all()), "sconv%dx%d%s, %s: out was written" % (ks, ks, form, what)
            out = torch.full((1, cout, hp, wp), 777.0, device="cuda:0")
            for bad in (pk[:-8].contiguous(), pk.float() if form else pk.bfloat16()):      # wrong size, wrong dtype
                with pytest.raises(lic.Lic360Error, match="packed must"):
                    conv(x, bad, b, sl, None, out, ring=2, **kw)
            torch.cuda.synchronize()
            assert bool((out == 777.0).all())
            with pytest.raises(lic.Lic360Error, match="packed must"):       # an unsupported channel count at the call: no pack of that shape exists
                conv(torch.zeros((1, 40, hp, wp), device="cuda:0"), pk, b, sl, None, out, ring=2, **kw)
            conv(x, pk, b, sl, None, out, ring=2, **kw)                     # and the good call still runs
            torch.cuda.synchronize()
            assert not bool((out == 777.0).all())


def test_fused_blocks_in_bf16x3_mode_match_the_oracle(lic, monkeypatch):
    """ResidualBlock / V2 / Down / Up at 192 channels in bf16x3 mode (fused path forced on a small map): the oracle's blocks to 1e-4, 16x closer
    than the oracle's blocks with bf16-rounded conv weights; every fused convolution runs on its bf16x3 form, none on lic360.sconv3x3"""
    import oracle as orc
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm)
    torch.manual_seed(6)
    c = 192
    x = _refresh(torch.randn((1, c, 12, 20), device="cuda:0")).contiguous()
    xn = x.cpu().numpy()
    rec = gs.SconvCalls(lic, monkeypatch)
    with torch.no_grad():
        for cls, fn, n3, n1 in ((lm.ResidualBlock, orc.blocks.residual, 1, 2), (lm.ResidualBlockV2, orc.blocks.residual_v2, 2, 0),
                                (lambda ch, d: lm.ResidualBlockDown(ch, ch, d), orc.blocks.residual_down, 1, 0), (lm.ResidualBlockUp, orc.blocks.residual_up, 2, 1)):
            blk = gs.jitter(cls(c, 0).to("cuda:0"))
            lm.set_conv_precision(blk, "bf16x3")
            rec.reset()
            got = blk(x.clone()).cpu().numpy()
            name = type(blk).__name__
            assert rec.only(sconv3x3_bf16x3=n3, sconv1x1_bf16x3=n1), (name, rec.made())
            p = _block_params(blk)
            want = fn(xn.copy(), p)
            p16 = {k: (_bf16(v) if k.endswith("weight") and np.ndim(v) == 4 else v) for k, v in p.items()}
            want16 = fn(xn.copy(), p16)
            err, err16 = float(np.abs(got - want).max()), float(np.abs(want16 - want).max())
            assert np.allclose(got, want, rtol=1e-4, atol=1e-4), "%s: max abs error %g" % (name, err)
            assert 16 * err <= err16, "%s: bf16x3 error %g, bf16 weights %g" % (name, err, err16)


def test_default_is_fp32_and_the_mode_switches_back(lic, monkeypatch):
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm)
    torch.manual_seed(7)
    c = 192
    x = _refresh(torch.randn((1, c, 12, 20), device="cuda:0")).contiguous()
    calls = gs.SconvCalls(lic, monkeypatch).counts
    with torch.no_grad():
        torch.manual_seed(8)
        ref = lm.ResidualBlockUp(c, 0).to("cuda:0")
        torch.manual_seed(8)
        blk = lm.ResidualBlockUp(c, 0).to("cuda:0")
        want = ref(x.clone())
        assert calls["sconv3x3_bf16x3"] == 0 and calls["sconv1x1_bf16x3"] == 0 and calls["sconv3x3"] == 2 and calls["sconv1x1"] == 1
        lm.set_conv_precision(blk, "bf16x3")
        b3 = blk(x.clone())
        assert calls["sconv3x3_bf16x3"] == 2 and calls["sconv1x1_bf16x3"] == 1
        lm.set_conv_precision(blk, "fp32")
        assert torch.equal(blk(x.clone()), want)
        assert not torch.equal(b3, want) and torch.allclose(b3, want, rtol=1e-4, atol=1e-4)
        lm.set_conv_precision(blk, "bf16x3")
        assert torch.equal(blk(x.clone()), b3)                              # each precision's pack is cached apart: switching never reuses the other's
    for bad in ("bf16", "FP32", None):
        with pytest.raises(ValueError):
            lm.set_conv_precision(blk, bad)


def test_whole_codec_in_bf16x3_mode_at_the_reference_width(lic, monkeypatch):
    """image -> analysis (bf16x3) -> fused entropy codecs -> bytes -> decode -> synthesis in both modes, 192 channels / 48 groups: the streams
    round-trip exactly; the synthesis of the decoded symbols in bf16x3 mode stays within 1e-4 of the fp32 one's range at the up-sampling stages
    (measured: 1e-5; the modes must differ there) and at the image (measured: equal -- the seeded networks' deep signal falls below the
    output's rounding).  Batch 2: the largest maps fill the chip (FUSED_MIN_FILL), so both transforms run fused convolutions in either mode."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
    import lic360_models as lm
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_main_params, make_imp_params
    calls = gs.SconvCalls(lic, monkeypatch).counts
    torch.manual_seed(12)
    C, G = 192, 48
    enc, dec = lm.CMP_Encoder(C, C, 8, 0).to("cuda:0").eval(), lm.CMP_Decoder(C, C, 8, 0).to("cuda:0").eval()
    lm.set_conv_precision(enc, "bf16x3")
    with torch.no_grad():
        dec.quant.weight.copy_(enc.quant.weight)
        img = torch.rand((2, 3, 512, 1024), device="cuda:0")
        code, mask, levels = enc(img)
    assert calls["sconv3x3_bf16x3"] > 0 and calls["sconv3x3"] == 0, calls
    assert tuple(code.shape) == (2, G, 64, 128) and tuple(levels.shape) == (2, 1, 32, 64)
    fc = FusedCodec(G, 64, 128, max_batch=2)
    fc.load_layers(make_main_params(5, G))
    ic = FusedImpCodec(32, 64, max_batch=2, hidden_channels=3 * G, nsym=G + 1)
    ic.load_layers(make_imp_params(5, cpg=3 * G, nsym=G + 1))
    streams, istreams = fc.encode(code.contiguous(), mask.contiguous()), ic.encode(levels.contiguous())
    lv2 = ic.decode(istreams)
    assert torch.equal(lv2, levels)
    mask2 = (torch.arange(G, device="cuda:0").view(1, G, 1, 1) < lv2.repeat_interleave(2, 2).repeat_interleave(2, 3)).float()
    code2 = fc.decode(streams, mask2)
    assert torch.equal(code2, code * mask)
    with torch.no_grad():
        stages, seen = (3, 5, 8, 9), {}                                   # the up-sampling stages and the last full-size ResidualBlockV2
        hooks = [dec.decoder.net[i].register_forward_hook(lambda m, a, o, i=i: seen.setdefault((getattr(dec.decoder.net[0], "_conv_precision", "fp32"), i), o.clone()))
                 for i in stages]
        n3 = calls["sconv3x3"]
        rec32 = dec(code2, mask2)
        assert calls["sconv3x3"] > n3, calls
        n3 = calls["sconv3x3_bf16x3"]
        lm.set_conv_precision(dec, "bf16x3")
        rec = dec(code2, mask2)
        assert calls["sconv3x3_bf16x3"] > n3, calls
        for h in hooks:
            h.remove()
    for i in stages:
        a, b = seen[("bf16x3", i)], seen[("fp32", i)]
        di, si = float((a - b).abs().max()), float(b.abs().max())
        print("synthesis stage %d: max |bf16x3 - fp32| = %g, max |fp32| = %g" % (i, di, si))
        assert di <= 1e-4 * si, (i, di, si)
    assert any(not torch.equal(seen[("bf16x3", i)], seen[("fp32", i)]) for i in stages)
    assert tuple(rec.shape) == (2, 3, 512, 1024) and bool(torch.isfinite(rec).all())
    d, scale = float((rec - rec32).abs().max()), float(rec32.abs().max())
    print("whole codec: max |bf16x3 - fp32| = %g, max |fp32| = %g, ratio %g" % (d, scale, d / scale))
    assert d <= 1e-4 * scale, (d, scale)
