"""The single-pass bf16 ("bf16x1") form of the transforms' sphere convolutions on real-valued data (lic360.sconv3x3_bf16x1 / sconv1x1_bf16x1,
lic360_models.set_conv_precision(m, "bf16x1")): single calls, the blocks at the reference width, mode switching, the whole codec.

The criterion of a call.  The contract is the fp32-accumulated convolution of the operands rounded once to bf16, so the statement to compare with is the
float64 convolution of the rounded x and w (tests/sconv_cases.py's reference, rounding by tests/sconv_bf16x1_cases.py's bit-level bf16_rne) at
rtol = atol = 1e-4 -- the project's bound for an fp32-accumulated kernel against a float64 statement of the same products -- and the form must really be
that one: 16 max |got - ref_bf16| <= max |ref_bf16 - ref_fp32| (the factor 16 is the bf16x3 test's, read the other way round: there the kernel has to be
16x closer to fp32 than single-pass bf16 is; here it has to be 16x closer to single-pass bf16 than fp32 is).

Chained layers.  Two correct summation orders of the same rounded products drift apart layer by layer (an input 1e-7 from a rounding boundary flips by a
whole bf16 step), so a chained run is not compared with a chained emulation cell by cell.  Each recorded call is held to the criterion on ITS OWN input
(teacher forcing), and a chained run is compared in its statistics: rms(out_bf16x1 - out_fp32) / rms(out_emulated - out_fp32) must lie in [0.9, 1.1],
the emulated run being the same module in fp32 mode with x and the weight rounded to bf16 in front of every stride-1 fused convolution.  The margin is
derived: truncation instead of rounding doubles the rms, rounding only one operand gives 0.71."""
import os
import sys

import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_bf16x1_cases as b1
import sconv_cases as sc
from gpu_support import lic  # noqa: F401
from util import _refresh

pytestmark = pytest.mark.gpu

STRIDE1 = ("sconv3x3", "sconv1x1", "sconv3x3_bf16x3", "sconv1x1_bf16x3", "sconv3x3_bf16x1", "sconv1x1_bf16x1")


def _window(c):
    r0, r1, c0, c1 = c.ring - c.crop, c.hp - c.ring - c.crop, c.ring_w - c.crop, c.wp - c.ring_w - c.crop
    k = 2 if c.shuffle else 1
    return (slice(None), slice(None), slice(k * r0, k * r1), slice(k * c0, k * c1))


def _criterion(case, data, got, what, frame=True):
    """gs.bf16x1_criterion against the float64 convolutions of the call's operands, rounded to bf16 and as given"""
    return gs.bf16x1_criterion(b1.reference(case, data), sc.reference(case, data), got, _window(case), sc.SENTINEL, what, frame)


def _call(lic, case, data):
    name = "sconv%dx%d_bf16x1" % (case.ks, case.ks)
    kw = dict(ring=case.ring, ring_w=case.ring_w, crop=case.crop, shuffle=case.shuffle)
    if case.ks == 3:
        kw.update(pad=case.pad, sphere=case.sphere)
    ops = (gs.dev(data["x"]), getattr(lic, name + "_pack")(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"]))
    return gs.sentinel_call(lambda out: getattr(lic, name)(*ops, out, **kw), sc.out_shape(case), sc.SENTINEL)


def _real_data(case, seed, wscale):
    rng = np.random.default_rng(seed)
    c = case
    f = lambda a: a.astype(np.float32)
    return dict(x=f(rng.standard_normal((c.n, c.cin, c.hp, c.wp))), w=f(rng.standard_normal((c.cout, c.cin, c.ks, c.ks)) * wscale),
                b=f(rng.standard_normal(c.cout)), slope=f(rng.random(c.cout)) if c.slope else None,
                res=f(rng.standard_normal(sc.out_shape(c))) if c.res else None)


# (cin, cout, hp, wp, ring, sphere, crop, act, residual, ring_w): the shapes of tests/test_gpu_sconv_bf16x3.py::CASES3
CASES3 = [(32, 96, 20, 36, 2, 1, 0, True, True, 2), (32, 384, 18, 34, 2, 0, 0, False, True, 2), (64, 96, 9, 70, 1, 1, 0, False, False, 1),
          (32, 192, 22, 40, 1, 1, 0, True, False, 2), (192, 192, 21, 37, 1, 2, 0, True, True, 2), (192, 192, 38, 24, 2, 1, 0, True, False, 2),
          (96, 96, 23, 40, 2, 1, 0, True, True, 2), (192, 192, 20, 36, 1, 1, 0, True, False, 2)]
SINGLE = [sc._c("c3_%dto%d_%dx%d_ring%d_%d_sphere%d" % (cin, cout, hp, wp, ring, ring_w, sphere), 3, cin, cout, 2, hp, wp, pad=2, sphere=sphere, ring=ring,
                ring_w=ring_w, crop=crop, slope=act, res=res) for cin, cout, hp, wp, ring, sphere, crop, act, res, ring_w in CASES3]
SINGLE += [sc._c("c3_shuffle_192to768_14x22", 3, 192, 768, 2, 14, 22, pad=2, sphere=1, ring=2, crop=1, shuffle=True)]       # ResidualBlockUp.conv1
SINGLE += [sc._c("c1_%dto%d_%dx%d" % (cin, cout, hp, wp), 1, cin, cout, 2, hp, wp, ring=ring, ring_w=ring_w, slope=act, res=res)
           for cin, cout, hp, wp, ring, ring_w, act, res in ((192, 96, 20, 36, 2, 2, True, False), (96, 192, 21, 37, 2, 2, False, True), (64, 384, 12, 20, 1, 3, True, True))]
SINGLE += [sc._c("c1_shuffled_shortcut_192to768_14x22", 1, 192, 768, 2, 14, 22, ring=2, crop=1, shuffle=True, slope=False, res=True)]   # ResidualBlockUp's shortcut


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: c.name)
def test_single_calls_are_the_convolution_of_rounded_operands(lic, case):
    assert getattr(lic, "sconv%dx%d_bf16x1_supported" % (case.ks, case.ks))(case.cin, case.cout)
    data = _real_data(case, case.cin + 7 * case.cout + case.hp, 0.05 if case.cout == 768 else 0.1)
    _criterion(case, data, _call(lic, case, data), case.name)


def test_each_form_takes_only_its_own_pack(lic):
    rng = np.random.default_rng(82)
    cin, cout, hp, wp = 64, 192, 20, 36
    x = torch.zeros((1, cin, hp, wp), device="cuda:0")
    b = torch.zeros(cout, device="cuda:0")
    for ks in (3, 1):
        w = torch.from_numpy(rng.standard_normal((cout, cin, ks, ks)).astype(np.float32)).cuda()
        f = lambda form, s="": getattr(lic, "sconv%dx%d%s%s" % (ks, ks, form, s))
        packs = {form: f(form, "_pack")(w) for form in ("", "_bf16x3", "_bf16x1")}
        kw = dict(pad=2, sphere=1) if ks == 3 else {}
        assert packs["_bf16x1"].dtype == torch.bfloat16 and packs["_bf16x1"].numel() * 2 == cout * cin * ks * ks * 2
        for form in packs:
            for other, pk in packs.items():
                out = torch.full((1, cout, hp, wp), 777.0, device="cuda:0")
                if other == form:
                    f(form)(x, pk, b, None, None, out, ring=2, **kw)
                    torch.cuda.synchronize()
                    assert not bool((out == 777.0).all())
                else:
                    with pytest.raises(lic.Lic360Error, match="packed must"):
                        f(form)(x, pk, b, None, None, out, ring=2, **kw)
                    torch.cuda.synchronize()
                    assert bool((out == 777.0).all()), "sconv%dx%d%s wrote out with the pack of %r" % (ks, ks, form, other)
        pk = packs["_bf16x1"]
        for bad in (pk[:-8].contiguous(), pk.float(), torch.cat([pk, pk])):   # wrong size, wrong dtype, the bf16x3 pack's size
            with pytest.raises(lic.Lic360Error, match="packed must"):
                f("_bf16x1")(x, bad, b, None, None, torch.zeros((1, cout, hp, wp), device="cuda:0"), ring=2, **kw)
        for ci, co in ((40, 192), (64, 100), (16, 96)):
            with pytest.raises(lic.Lic360Error, match="not supported"):
                f("_bf16x1", "_pack")(torch.zeros((co, ci, ks, ks), device="cuda:0"))
    assert not lic.sconv3x3_bf16x1_supported(16, 192) and not lic.sconv1x1_bf16x1_supported(48, 96)


def _instrument(lic, monkeypatch):
    """the recorder with the weight behind every pack, bf16x1 calls recorded while `recording` and -- while `emulating` -- x and the weight rounded to bf16 in
    front of the fp32 stride-1 calls"""
    return gs.SconvCalls(lic, monkeypatch, emulate=("sconv3x3", "sconv1x1"), record=True)


def _check_record(rec, what):
    """a recorded bf16x1 call held to the single-call criterion on its own input (window only: `out` was a scratch buffer)"""
    name, (x, bias, slope, res), w, kw, out = rec
    ks = 3 if "3x3" in name else 1
    n, cin, hp, wp = x.shape
    ring = kw.get("ring", 1 if ks == 3 else 2)
    sphere = int(kw.get("sphere", True)) if ks == 3 else 0
    case = sc.Case(what, ks, cin, w.shape[0], n, hp, wp, kw.get("pad", 2) if ks == 3 else 0, sphere, ring, ring if kw.get("ring_w") is None else kw["ring_w"],
                   kw.get("crop", 0), bool(kw.get("shuffle", False)), slope is not None, res is not None, False)
    num = lambda t: None if t is None else t.cpu().numpy()
    data = dict(x=num(x), w=num(w).reshape(w.shape[0], cin, ks, ks), b=num(bias), slope=num(slope), res=num(res))
    assert tuple(out.shape) == sc.out_shape(case)
    return _criterion(case, data, out.cpu().numpy(), what, frame=False)


def test_fused_blocks_in_bf16x1_mode(lic, monkeypatch):
    """ResidualBlock / V2 / Down / Up at 192 channels (fused path forced on a small map): every stride-1 fused layer on its bf16x1 form and none on the
    others; every recorded call within the single-call criterion on its own input; the block's rms deviation from fp32 that of the emulated run"""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm)
    ins = _instrument(lic, monkeypatch)
    torch.manual_seed(6)
    c = 192
    x = _refresh(torch.randn((1, c, 12, 20), device="cuda:0")).contiguous()
    with torch.no_grad():
        for cls, n3, n1 in ((lm.ResidualBlock, 1, 2), (lm.ResidualBlockV2, 2, 0), (lambda ch, d: lm.ResidualBlockDown(ch, ch, d), 1, 0), (lm.ResidualBlockUp, 2, 1)):
            blk = gs.jitter(cls(c, 0).to("cuda:0"))
            name = type(blk).__name__
            ins.reset()
            out32 = blk(x.clone())
            assert ins.only(sconv3x3=n3, sconv1x1=n1), (name, ins.made())
            ins.reset()
            ins.emulating = True
            emu = blk(x.clone())
            ins.emulating = False
            assert ins.only(sconv3x3=n3, sconv1x1=n1), (name, ins.made())
            lm.set_conv_precision(blk, "bf16x1")
            ins.reset()
            ins.recording = True
            got = blk(x.clone())
            ins.recording = False
            assert ins.only(sconv3x3_bf16x1=n3, sconv1x1_bf16x1=n1), (name, ins.made())
            assert len(ins.records) == n3 + n1
            for i, rec in enumerate(ins.records):
                _check_record(rec, "%s call %d (%s)" % (name, i, rec[0]))
            assert got.shape == out32.shape and bool(torch.isfinite(got).all()) and not torch.equal(got, out32)
            gs.bf16x1_ratio(got, emu, out32, name)


def test_mode_switching(lic, monkeypatch):
    """fp32 -> bf16x1 -> bf16x3 -> fp32 -> bf16x1 on one block: each mode's output equals its own earlier output bit for bit (each precision's pack is
    cached apart) and differs from the others'; the default is fp32; unknown names raise"""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm)
    ins = _instrument(lic, monkeypatch)
    torch.manual_seed(7)
    c = 192
    x = _refresh(torch.randn((1, c, 12, 20), device="cuda:0")).contiguous()
    with torch.no_grad():
        blk = lm.ResidualBlockUp(c, 0).to("cuda:0")
        first = {}
        for mode in (None, "bf16x1", "bf16x3", "fp32", "bf16x1"):
            if mode is not None:
                lm.set_conv_precision(blk, mode)
            mode = mode or "fp32"
            ins.reset()
            out = blk(x.clone())
            suffix = "" if mode == "fp32" else "_" + mode
            assert ins.only(**{"sconv3x3" + suffix: 2, "sconv1x1" + suffix: 1}), (mode, ins.made())
            if mode in first:
                assert torch.equal(out, first[mode]), mode
            else:
                for other, o in first.items():
                    assert not torch.equal(out, o), (mode, other)
                first[mode] = out
        assert set(first) == {"fp32", "bf16x1", "bf16x3"}
        assert gs.rms(first["bf16x3"] - first["fp32"]) * 16 < gs.rms(first["bf16x1"] - first["fp32"])
    for bad in ("bf16", "FP32", None):
        with pytest.raises(ValueError):
            lm.set_conv_precision(blk, bad)


def test_whole_codec_in_bf16x1_mode_at_the_reference_width(lic, monkeypatch):
    """image -> analysis (bf16x1) -> fused entropy codecs -> bytes -> decode -> synthesis in fp32, bf16x1 and emulated, 192 channels / 48 groups, batch 2:
    both streams round-trip exactly whatever arithmetic the analysis transform ran in; the stride-2 layers run on the fp32 stride-2 kernels; the bf16x1
    synthesis differs from the fp32 one at the up-sampling stages and the last full-size ResidualBlockV2 (3, 5, 8, 9) by the emulated run's rms.  At batch 2
    the maps up to 68 x 132 have fewer than FUSED_MIN_WORKGROUPS tiles (2 x 4 x 8 = 64; the 192 -> 768 layer at 36 x 68: 2 x 2 x 4 x 4 = 64), so everything up to
    and including stage 3 is library work in every mode: there both deviations are zero and the ratio is undefined, and the stage's three outputs must be EQUAL
    bit for bit instead; which stages have a fused convolution upstream is read off the call counter when the stage's hook fires, not off the outputs, and
    stages 5, 8 and 9 must (the 192 -> 768 layer at 68 x 132 and every layer from 132 x 260 on have 256 tiles or more).  The image itself is not gated: with
    seeded weights the deep signal falls below the output's rounding (tests/test_gpu_sconv_bf16x3.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
    import lic360_models as lm
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_main_params, make_imp_params
    ins = _instrument(lic, monkeypatch)
    torch.manual_seed(12)
    C, G = 192, 48
    enc, dec = lm.CMP_Encoder(C, C, 8, 0).to("cuda:0").eval(), lm.CMP_Decoder(C, C, 8, 0).to("cuda:0").eval()
    lm.set_conv_precision(enc, "bf16x1")
    with torch.no_grad():
        dec.quant.weight.copy_(enc.quant.weight)
        img = torch.rand((2, 3, 512, 1024), device="cuda:0")
        code, mask, levels = enc(img)
    calls = ins.counts
    assert calls["sconv3x3_bf16x1"] > 0 and calls["sconv1x1_bf16x1"] > 0, calls
    assert calls["sconv3x3"] == 0 and calls["sconv1x1"] == 0 and calls["sconv3x3_bf16x3"] == 0 and calls["sconv1x1_bf16x3"] == 0, calls
    assert calls["sconv3x3s2"] > 0 and calls["sconv1x1s2"] > 0, calls        # the stride-2 layers: the fp32 stride-2 kernels, as in bf16x3 mode
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
        stages, seen, run, upstream = (3, 5, 8, 9), {}, {}, {}

        def keep(i, o):
            seen[(run["label"], i)] = o.clone()
            upstream[(run["label"], i)] = sum(calls[k] for k in STRIDE1)    # stride-1 fused convolutions of this run so far

        hooks = [dec.decoder.net[i].register_forward_hook(lambda m, a, o, i=i: keep(i, o)) for i in stages]
        ins.reset()
        run["label"] = "fp32"
        rec32 = dec(code2, mask2)
        assert calls["sconv3x3"] > 0 and calls["sconv3x3_bf16x1"] == 0, calls
        n32 = dict(calls)
        ins.reset()
        run["label"], ins.emulating = "emulated", True
        dec(code2, mask2)
        ins.emulating = False
        assert dict(calls) == n32
        lm.set_conv_precision(dec, "bf16x1")
        ins.reset()
        run["label"] = "bf16x1"
        rec = dec(code2, mask2)
        assert calls["sconv3x3_bf16x1"] == n32["sconv3x3"] and calls["sconv1x1_bf16x1"] == n32["sconv1x1"] and calls["sconv3x3"] == 0 and calls["sconv1x1"] == 0, calls
        for h in hooks:
            h.remove()
    assert tuple(rec.shape) == (2, 3, 512, 1024) and bool(torch.isfinite(rec).all()) and tuple(rec32.shape) == tuple(rec.shape)
    assert len(seen) == 3 * len(stages)
    for i in stages:
        assert upstream[("bf16x1", i)] == upstream[("fp32", i)] == upstream[("emulated", i)], (i, upstream)
        if upstream[("bf16x1", i)] == 0:                                    # library work only so far: one arithmetic in every mode
            assert i == 3, (i, upstream)
            print("synthesis stage %d: no fused convolution upstream at this batch; the three runs must be equal" % i)
            assert torch.equal(seen[("bf16x1", i)], seen[("fp32", i)]) and torch.equal(seen[("emulated", i)], seen[("fp32", i)]), i
            continue
        assert not torch.equal(seen[("bf16x1", i)], seen[("fp32", i)]), i
        gs.bf16x1_ratio(seen[("bf16x1", i)], seen[("emulated", i)], seen[("fp32", i)], "synthesis stage %d" % i)
    assert all(upstream[("bf16x1", i)] > 0 for i in (5, 8, 9)), upstream
    print("whole codec: max |bf16x1 - fp32| at the image = %g, max |fp32| = %g" % (float((rec - rec32).abs().max()), float(rec32.abs().max())))
