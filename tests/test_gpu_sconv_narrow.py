"""set_conv_precision(.., small="narrow") inside the transforms: the blocks at 192 channels on the maps whose launches have too few workgroups for the wide kernels --
36 x 68 at batch 8, 132 x 260 at batch 1 -- with the real count rule (nothing forced).  With the keyword on, the routed layers make the expected narrow calls and no
library convolution; the output is, bit for bit, what the WIDE kernels give on the same map (forced there by dropping the count rule) -- in bf16x3 and bf16x1 that
is the whole check: the wide kernels are held to their bounds by the forms' own files -- and in fp32 also within 1e-4 of the library path (the bound of
tests/test_gpu_models.py); "narrow" ->
"library" -> "narrow" and a never-set module give the library path's bits; a recorded gradient, a non-contiguous x and a missing bias run the library path; a map
the wide kernel takes makes no narrow call; whole transforms at batch 1 with every keyword on, through the entropy codecs."""
import pytest
import torch

import gpu_support as gs
from gpu_support import lic  # noqa: F401
from util import _refresh

pytestmark = pytest.mark.gpu

FORMS = ("fp32", "bf16x3", "bf16x1")
NARROW = ("sconv3x3_narrow", "sconv1x1_narrow", "sconv1x1_gate_narrow")


def _calls(lic, monkeypatch):
    """every lic360.sconv* call counted, the narrow calls' keywords, and every nn.Conv2d forward that reaches the library"""
    return gs.SconvCalls(lic, monkeypatch, narrow=True, library=True)


def _make(lm, kind, seed=31):
    torch.manual_seed(seed)
    c = 192
    blk = {"ResidualBlock": lambda: lm.ResidualBlock(c, 0), "ResidualBlockV2": lambda: lm.ResidualBlockV2(c, 0), "AttentionBlock": lambda: lm.AttentionBlock(c, 0),
           "ResidualBlockUp": lambda: lm.ResidualBlockUp(c, 0), "ResidualBlockDown": lambda: lm.ResidualBlockDown(c, c, 0)}[kind]().to("cuda:0").eval()
    return gs.jitter(blk)


def _sfx(p):
    return "" if p == "fp32" else "_" + p


# (block, input map, precision -> the narrow calls {name: count} and cpw values expected, other native calls expected); None: the block stays on the library.
# Batch 1, 132 x 260 (128 tiles): 192-channel layers at cpw 96 (256 workgroups), 96-channel layers at cpw 48.  Batch 8, 36 x 68 (64 tiles): 192-channel layers at
# cpw 48 (256 workgroups); the bottleneck's 96 -> 96 layer reaches 128 and stays on the library, and with it the attention block; in bf16x3 the 34-row window of
# ResidualBlockV2.conv1 has no tall last row at cpw 48: 3 tile rows, 384 workgroups, 75 % of two rounds -- below FUSED_MIN_FILL, so that block stays on the library.
# Routed back by measurement (lic360_models.NARROW_ROUTED_BACK): ResidualBlockV2 on 132 x 260 at batch 1 in fp32.
def _expect(kind, n, precision):
    s2 = ""                                                                 # (the stride-2 layers follow the stride2= keyword, left at fp32 here)
    if n == 1:
        return {"ResidualBlock": (dict(sconv3x3_narrow=1, sconv1x1_narrow=2), {48, 96}, {}),
                "ResidualBlockV2": None if precision == "fp32" else (dict(sconv3x3_narrow=2), {96}, {}),      # fp32: conv1's tall row at cpw 96, NARROW_ROUTED_BACK
                "AttentionBlock": (dict(sconv3x3_narrow=6, sconv1x1_narrow=12, sconv1x1_gate_narrow=1), {48, 96}, {}),
                "ResidualBlockUp": (dict(sconv3x3_narrow=2, sconv1x1_narrow=1), {96}, {}),
                "ResidualBlockDown": (dict(sconv3x3_narrow=1), {96}, {"sconv3x3s2" + s2: 1, "sconv1x1s2" + s2: 1})}[kind]
    return {"ResidualBlock": None, "AttentionBlock": None, "ResidualBlockUp": (dict(), set(), {"sconv3x3" + _sfx(precision): 2, "sconv1x1" + _sfx(precision): 1}),
            "ResidualBlockV2": None if precision == "bf16x3" else (dict(sconv3x3_narrow=2), {48}, {}),
            "ResidualBlockDown": (dict(sconv3x3_narrow=1), {48}, {})}[kind]


def _input(kind, n):
    hp, wp = (36, 68) if n == 8 else (132, 260)
    if kind == "ResidualBlockDown":                                         # its conv2 runs on the down-sampled map
        hp, wp = 2 * (hp - 4) + 4, 2 * (wp - 4) + 4
    if kind == "ResidualBlockUp" and n == 1:                                # conv1 and the shortcut on 68 x 132 (128 wide workgroups), conv2 on 132 x 260
        hp, wp = 68, 132
    return _refresh(torch.randn((n, 192, hp, wp), device="cuda:0")).contiguous()


@pytest.mark.parametrize("n", (1, 8))
@pytest.mark.parametrize("kind", ("ResidualBlock", "ResidualBlockV2", "AttentionBlock", "ResidualBlockUp", "ResidualBlockDown"))
def test_the_blocks_route_small_launches_to_narrow_workgroups(lic, monkeypatch, kind, n):
    import lic360_models as lm
    torch.manual_seed(5)
    x = _input(kind, n)
    blk = _make(lm, kind)
    calls = _calls(lic, monkeypatch)
    with torch.no_grad():
        never_set = blk(x.clone())
        library_convs = list(calls.library)
        assert not any(calls.counts[k] for k in NARROW)
        for precision in FORMS:
            expect = _expect(kind, n, precision)
            lm.set_conv_precision(blk, precision, gate="fused")
            calls.reset()
            lib = blk(x.clone())
            assert not any(calls.counts[k] for k in NARROW), calls.made()
            lib_made, lib_library = calls.made(), list(calls.library)
            if precision == "fp32" and kind != "AttentionBlock":
                assert torch.equal(lib, never_set) and lib_library == library_convs           # "library", and never set: the parent's path
            lm.set_conv_precision(blk, precision, gate="fused", small="narrow")
            calls.reset()
            got = blk(x.clone())
            made = calls.made()
            print(kind, n, precision, made, sorted(set(calls.kw)), "library convs:", calls.library)
            if expect is None:                                              # the count rule keeps the block on the library
                assert made == lib_made and calls.library == lib_library and torch.equal(got, lib)
                continue
            narrow, cpws, others = expect
            assert {k: v for k, v in made.items() if k in NARROW} == narrow, made
            assert {k: v for k, v in made.items() if k not in NARROW} == others, made
            assert {c for _, _, c in calls.kw} == cpws and {f for _, f, _ in calls.kw} <= {precision}, calls.kw
            stride1 = [c for c in calls.library if c[3] == 1]
            assert not stride1, stride1                                     # no library convolution for the routed layers
            assert [c for c in calls.library if c[3] == 2] == ([] if others or kind != "ResidualBlockDown" else [(192, 192, 1, 2), (192, 192, 3, 2)])
            # the wide kernels on the same map: the same bits
            gs.count_rule(monkeypatch, lm)                                  # dropped: with small="library" every layer runs on the wide kernels
            lm.set_conv_precision(blk, precision, gate="fused")
            calls.reset()
            wide = blk(x.clone())
            assert not any(calls.counts[k] for k in NARROW) and sum(calls.counts.values()) == sum(narrow.values()) + sum(others.values()), calls.made()
            gs.count_rule(monkeypatch, lm, on=False)
            assert torch.equal(got, wide), (kind, n, precision, float((got - wide).abs().max()))
            if precision == "fp32":
                assert torch.allclose(got, lib, rtol=1e-4, atol=1e-4), float((got - lib).abs().max())
            assert narrow == {} or not torch.equal(got, lib)
            # "narrow" -> "library" -> "narrow"
            lm.set_conv_precision(blk, precision, gate="fused")
            assert torch.equal(blk(x.clone()), lib)
            lm.set_conv_precision(blk, precision, gate="fused", small="narrow")
            assert torch.equal(blk(x.clone()), got)


def test_the_library_path_runs_outside_the_other_conditions(lic, monkeypatch):
    import lic360_models as lm
    x = _input("ResidualBlockV2", 8)                                        # 36 x 68 at batch 8: both layers at cpw 48 in fp32
    blk = lm.set_conv_precision(_make(lm, "ResidualBlockV2"), "fp32", small="narrow")
    calls = _calls(lic, monkeypatch)

    def library(run):
        calls.reset()
        out = run()
        assert not calls.made() and len(calls.library) == 2, (calls.made(), calls.library)
        return out

    with torch.no_grad():
        got = blk(x.clone())
        assert calls.made() == dict(sconv3x3_narrow=2)                      # (the conditions hold here)
    library(lambda: blk(x.clone().requires_grad_()))                        # a recorded gradient: on x, on the parameters
    library(lambda: blk(x.clone()))
    with torch.no_grad():
        xt = x.clone().to(memory_format=torch.channels_last)                # a non-contiguous x
        assert not xt.is_contiguous()
        out = library(lambda: blk(xt))
        assert torch.allclose(out, got, rtol=1e-4, atol=1e-4)
        bias = blk.conv1.bias                                               # a missing bias
        blk.conv1.bias = None
        library(lambda: blk(x.clone()))
        blk.conv1.bias = bias
        calls.reset()
        assert torch.equal(blk(x.clone()), got) and calls.made() == dict(sconv3x3_narrow=2)
        # a map the wide kernel takes makes no narrow call
        big = _refresh(torch.randn((1, 192, 260, 516), device="cuda:0")).contiguous()
        calls.reset()
        blk(big)
        assert calls.made() == dict(sconv3x3=2)
        # a 48-channel block: a shape the kernels do not take
        torch.manual_seed(3)
        small = lm.set_conv_precision(lm.ResidualBlockV2(48, 0).to("cuda:0").eval(), "fp32", small="narrow")
        calls.reset()
        small(_refresh(torch.randn((1, 48, 132, 260), device="cuda:0")).contiguous())
        assert not calls.made() and len(calls.library) == 2


def test_whole_transforms_at_batch_1_with_every_keyword(lic, monkeypatch):
    """image -> analysis -> fused entropy codecs -> bytes -> decode -> synthesis at 192 channels / 48 groups, batch 1, the real count rule, the fast mode with every
    keyword on: the 132 x 260 stage runs on narrow workgroups, no stride-1 192- or 96-channel layer of that stage reaches the library, the latent codes and decodes
    to the same symbols, the image is finite"""
    import lic360_models as lm
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_main_params, make_imp_params
    calls = _calls(lic, monkeypatch)
    torch.manual_seed(12)
    C, G = 192, 48
    kw = dict(stride2="bf16x1", gdn="bf16x3", gate="fused", small="narrow")
    enc = lm.set_conv_precision(lm.CMP_Encoder(C, C, 8, 0).to("cuda:0").eval(), "bf16x1", **kw)
    dec = lm.set_conv_precision(lm.CMP_Decoder(C, C, 8, 0).to("cuda:0").eval(), "bf16x1", **kw)
    with torch.no_grad():
        img = torch.rand((1, 3, 512, 1024), device="cuda:0")
        code, mask, levels = enc(img)
        # stage 2 of the analysis side: ResidualBlockDown.conv2, the attention block (18 layers + gate), ResidualBlockV2 (2)
        assert {k: calls.counts[k] for k in NARROW} == dict(sconv3x3_narrow=1 + 6 + 2, sconv1x1_narrow=12, sconv1x1_gate_narrow=1), calls.made()
        assert {(f, c) for _, f, c in calls.kw} == {("bf16x1", 96), ("bf16x1", 48)}
        assert calls.counts["sconv3x3s2_bf16x1"] == 1 and calls.counts["sconv1x1s2"] == 1, calls.made()      # stage 2's stride-2 layers went with their block
        assert tuple(code.shape) == (1, G, 64, 128) and tuple(levels.shape) == (1, 1, 32, 64) and bool(torch.isfinite(code).all())
        fc = FusedCodec(G, 64, 128, max_batch=1)
        fc.load_layers(make_main_params(5, G))
        ic = FusedImpCodec(32, 64, max_batch=1, hidden_channels=3 * G, nsym=G + 1)
        ic.load_layers(make_imp_params(5, cpg=3 * G, nsym=G + 1))
        streams, istreams = fc.encode(code.contiguous(), mask.contiguous()), ic.encode(levels.contiguous())
        lv2 = ic.decode(istreams)
        assert torch.equal(lv2, levels)
        mask2 = (torch.arange(G, device="cuda:0").view(1, G, 1, 1) < lv2.repeat_interleave(2, 2).repeat_interleave(2, 3)).float()
        code2 = fc.decode(streams, mask2)
        assert torch.equal(code2, code * mask)
        calls.reset()
        image = dec(code2, mask2)
        # the synthesis side: Up (68 x 132 -> 132 x 260: conv1, shortcut, conv2), ResidualBlockV2 at 132 x 260, the attention block there, ResidualBlockV2
        print("decoder:", calls.made(), sorted(set(calls.kw)))
        assert {k: calls.counts[k] for k in NARROW} == dict(sconv3x3_narrow=2 + 6 + 2, sconv1x1_narrow=1 + 12, sconv1x1_gate_narrow=1), calls.made()
        assert tuple(image.shape) == (1, 3, 512, 1024) and bool(torch.isfinite(image).all())
