"""The single-pass bf16 forms of the stride-2 sphere convolutions on real-valued data (lic360.sconv3x3s2_bf16x1 / sconv1x1s2_bf16x1,
lic360_models.set_conv_precision(m, precision, stride2="bf16x1")): single calls at the production shapes, the down-sampling blocks at the reference
width, the default mode, mode switching, the whole analysis transform.

The criteria are tests/test_gpu_sconv_bf16x1.py's, and they are not restated here: gpu_support.bf16x1_criterion and bf16x1_ratio run as they stand, the
single call with this form's two float64 references and the output's interior as the window.  A call: the float64 stride-2 convolution of the operands rounded once to bf16
(tests/sconv_s2_cases.py's reference behind tests/sconv_bf16x1_cases.py's bit-level bf16_rne) at rtol = atol = 1e-4, and the form must really be that one:
16 max |got - ref_bf16| <= max |ref_bf16 - ref_fp32|.  A chained run: rms(out_bf16x1 - out_fp32) / rms(out_emulated - out_fp32) in [0.9, 1.1], the
emulated run being the same module in fp32 with x and the weight rounded to bf16 in front of every stride-2 fused convolution (truncation instead of
rounding doubles the rms, rounding only one operand gives 0.71)."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_s2_bf16x1_cases as sb
import sconv_s2_cases as s2
from gpu_support import lic  # noqa: F401
from util import _refresh

pytestmark = pytest.mark.gpu

S2_FP32 = ("sconv3x3s2", "sconv1x1s2")
S2_B1 = ("sconv3x3s2_bf16x1", "sconv1x1s2_bf16x1")


def _real_data(case, seed, wscale=0.1):
    rng = np.random.default_rng(seed)
    c = case
    f = lambda a: a.astype(np.float32)
    return dict(x=f(rng.standard_normal((c.n, c.cin, c.hp, c.wp))), w=f(rng.standard_normal((c.cout, c.cin, c.ks, c.ks)) * wscale),
                b=f(rng.standard_normal(c.cout)), slope=f(rng.random(c.cout)) if c.slope else None,
                res=f(rng.standard_normal(s2.out_shape(c))) if c.res else None)


@pytest.mark.parametrize("case", sb.PRODUCTION, ids=lambda c: c.name)
def test_single_calls_are_the_stride_2_convolution_of_rounded_operands(lic, case):
    assert (lic.sconv3x3s2_bf16x1_supported if case.ks == 3 else lic.sconv1x1s2_bf16x1_supported)(case.cin, case.cout)
    data = _real_data(case, case.hp + 7 * case.ks)
    conv, pack = (lic.sconv3x3s2_bf16x1, lic.sconv3x3_bf16x1_pack) if case.ks == 3 else (lic.sconv1x1s2_bf16x1, lic.sconv1x1_bf16x1_pack)
    kw = dict(pad=case.pad, oring=case.oring, **(dict(sphere=bool(case.sphere)) if case.ks == 3 else {}))
    ops = (gs.dev(data["x"]), pack(gs.dev(data["w"])), gs.dev(data["b"]), gs.dev(data["slope"]), gs.dev(data["res"]))
    (n, co, ohp, owp), r = s2.out_shape(case), case.oring
    got = gs.sentinel_call(lambda out: conv(*ops, out, **kw), (n, co, ohp, owp), s2.SENTINEL)
    window = (slice(None), slice(None), slice(r, ohp - r), slice(r, owp - r))                       # the output's interior: no crop, no shuffle
    # the float64 stride-2 convolution of the rounded operands and of the operands as given: window at 1e-4 and 16x closer than fp32; the frame untouched
    gs.bf16x1_criterion(sb.reference(case, data), s2.reference(case, data), got, window, s2.SENTINEL, case.name)


def _instrument(lic, monkeypatch):
    """the recorder with the weight behind every pack and -- while `emulating` -- x and the weight rounded to bf16 in front of the fp32 stride-2 calls"""
    return gs.SconvCalls(lic, monkeypatch, emulate=S2_FP32)


def _blocks(lm):
    """the two kinds of module with a fused stride-2 layer at 192 channels, and their stride-2 calls (3x3, 1x1)"""
    torch.manual_seed(16)
    out = []
    for make, n3, n1 in ((lambda: lm.ResidualBlockDown(192, 192, 0), 1, 1), (lambda: lm.SphereConv2(192, 192, 3, 2, 3, 0), 1, 0)):
        out.append((gs.jitter(make().to("cuda:0").eval()), n3, n1))
    return out


def _counts(ins, fp32=(0, 0), b1=(0, 0)):
    """the four stride-2 entry points alone: the blocks' stride-1 conv2 is counted too, on the entry point of the mode the test is in"""
    return {k: ins.counts[k] for k in S2_FP32 + S2_B1} == dict(zip(S2_FP32 + S2_B1, fp32 + b1))


def _input():
    torch.manual_seed(17)
    return _refresh(torch.randn((1, 192, 36, 68), device="cuda:0")).contiguous()


def test_blocks_with_stride2_bf16x1(lic, monkeypatch):
    """ResidualBlockDown and SphereConv2 at 192 channels (fused path forced on a small map): with the keyword every fused stride-2 layer runs on the new entry
    points and none on the fp32 stride-2 ones, and the block's rms deviation from its fp32 output is that of the emulated run"""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    ins = _instrument(lic, monkeypatch)
    x = _input()
    with torch.no_grad():
        for blk, n3, n1 in _blocks(lm):
            name = type(blk).__name__
            ins.reset()
            out32 = blk(x.clone())
            assert _counts(ins, fp32=(n3, n1)), (name, ins.made())
            ins.reset()
            ins.emulating = True
            emu = blk(x.clone())
            ins.emulating = False
            assert _counts(ins, fp32=(n3, n1)), (name, ins.made())
            assert lm.set_conv_precision(blk, "fp32", stride2="bf16x1") is blk
            ins.reset()
            got = blk(x.clone())
            assert _counts(ins, b1=(n3, n1)), (name, ins.made())
            assert got.shape == out32.shape == (1, 192, 20, 36) and bool(torch.isfinite(got).all()) and not torch.equal(got, out32)
            gs.bf16x1_ratio(got, emu, out32, name)
            for c in (blk.conv1, blk.short_cut) if n1 else (blk.conv,):   # the pack is the stride-1 form's, under its key
                assert set(c._sconv_packs) == {"fp32", "bf16x1"} and c._sconv_packs["bf16x1"][1].dtype == torch.bfloat16


def test_without_the_keyword_nothing_changes(lic, monkeypatch):
    """in "fp32", "bf16x3" and "bf16x1" mode the same blocks make the fp32 stride-2 calls and equal, bit for bit, the run of the block whose modules were
    given the mode the way the setter did before the keyword existed (no _stride2_precision attribute anywhere) -- also after the keyword was on and off
    again"""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    ins = _instrument(lic, monkeypatch)
    x = _input()
    with torch.no_grad():
        for blk, n3, n1 in _blocks(lm):
            for mode in lm.CONV_PRECISIONS:
                for m in blk.modules():                                     # a run that never touched the keyword
                    m._conv_precision = mode
                    m.__dict__.pop("_stride2_precision", None)
                    assert not hasattr(m, "_stride2_precision")
                ins.reset()
                want = blk(x.clone())
                assert _counts(ins, fp32=(n3, n1)), (mode, ins.made())
                lm.set_conv_precision(blk, mode)
                assert all(m._stride2_precision == "fp32" for m in blk.modules())
                ins.reset()
                assert torch.equal(blk(x.clone()), want) and _counts(ins, fp32=(n3, n1)), (mode, ins.made())
                lm.set_conv_precision(blk, mode, stride2="bf16x1")
                assert not torch.equal(blk(x.clone()), want)
                lm.set_conv_precision(blk, mode)
                ins.reset()
                assert torch.equal(blk(x.clone()), want) and _counts(ins, fp32=(n3, n1)), (mode, ins.made())


def test_switching_stride2_on_off_on(lic, monkeypatch):
    """on -> off -> on -> off on one block, in "bf16x1" mode: each setting's output equals its own earlier output bit for bit (each form's pack is cached
    apart) and differs from the other's"""
    import lic360_models as lm
    gs.count_rule(monkeypatch, lm, stride2=True)
    ins = _instrument(lic, monkeypatch)
    x = _input()
    with torch.no_grad():
        for blk, n3, n1 in _blocks(lm):
            first = {}
            for s2p in ("bf16x1", "fp32", "bf16x1", "fp32"):
                lm.set_conv_precision(blk, "bf16x1", stride2=s2p)
                ins.reset()
                out = blk(x.clone())
                assert _counts(ins, **{"b1" if s2p == "bf16x1" else "fp32": (n3, n1)}), (s2p, ins.made())
                if s2p in first:
                    assert torch.equal(out, first[s2p]), s2p
                else:
                    first[s2p] = out
            assert not torch.equal(first["fp32"], first["bf16x1"])


def test_the_large_shortcut_is_routed_to_fp32(lic, monkeypatch):
    """the one production shape on which the bf16x1 form did not beat the fp32 kernel by more than the spreads (the 1x1 shortcut on the 260 x 516 map,
    DESIGN 7c''') stays on fp32 with the keyword on; the 3x3 beside it and the shortcut on the 132 x 260 map do not"""
    import lic360_models as lm
    ins = _instrument(lic, monkeypatch)
    with torch.no_grad():
        blk = lm.set_conv_precision(lm.ResidualBlockDown(192, 192, 0).to("cuda:0").eval(), "bf16x1", stride2="bf16x1")
        for hp, wp, n, want in ((260, 516, 2, dict(fp32=(0, 1), b1=(1, 0))), (132, 260, 8, dict(b1=(1, 1)))):
            assert (hp * wp <= lm.S2_BF16X1_1X1_MAX_CELLS) == (want.get("fp32") is None)
            ins.reset()
            out = blk(torch.randn((n, 192, hp, wp), device="cuda:0"))
            assert _counts(ins, **want), (hp, wp, ins.made())
            assert tuple(out.shape) == (n, 192, (hp - 4) // 2 + 4, (wp - 4) // 2 + 4) and bool(torch.isfinite(out).all())


def test_whole_analysis_transform_with_stride2_bf16x1(lic, monkeypatch):
    """image -> analysis ("bf16x1" + stride2="bf16x1"), 192 channels / 48 groups, batch 2 -> fused entropy codecs -> bytes -> decode: the latent is coded and
    decodes to the same symbols.  At batch 2 stage 2's stride-2 layers have 256 tiles and run fused (its conv1 on the new 3x3 form, its 260 x 516 shortcut
    on fp32 by the measured route); stage 3 and SphereConv2 (64 and 16 tiles) are library work, as in every mode.  So what this test pins of the new forms inside the
    network is ONE call, stage 2's conv1 (`b1=(1, 0)`); the new 1x1 and the small-map 3x3 run inside a module only in the block tests above, with the gates
    forced open."""
    import lic360_models as lm
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_main_params, make_imp_params
    ins = _instrument(lic, monkeypatch)
    torch.manual_seed(12)
    C, G = 192, 48
    enc = lm.CMP_Encoder(C, C, 8, 0).to("cuda:0").eval()
    lm.set_conv_precision(enc, "bf16x1", stride2="bf16x1")
    with torch.no_grad():
        img = torch.rand((2, 3, 512, 1024), device="cuda:0")
        code, mask, levels = enc(img)
    assert _counts(ins, fp32=(0, 1), b1=(1, 0)), ins.made()
    assert tuple(code.shape) == (2, G, 64, 128) and tuple(levels.shape) == (2, 1, 32, 64) and bool(torch.isfinite(code).all())
    fc = FusedCodec(G, 64, 128, max_batch=2)
    fc.load_layers(make_main_params(5, G))
    ic = FusedImpCodec(32, 64, max_batch=2, hidden_channels=3 * G, nsym=G + 1)
    ic.load_layers(make_imp_params(5, cpg=3 * G, nsym=G + 1))
    streams, istreams = fc.encode(code.contiguous(), mask.contiguous()), ic.encode(levels.contiguous())
    lv2 = ic.decode(istreams)
    assert torch.equal(lv2, levels)
    mask2 = (torch.arange(G, device="cuda:0").view(1, G, 1, 1) < lv2.repeat_interleave(2, 2).repeat_interleave(2, 3)).float()
    assert torch.equal(fc.decode(streams, mask2), code * mask)
