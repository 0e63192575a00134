"""The attention blocks' fused gate on real data and inside the transforms.  Single calls of the three forms against the float64 gate of the operands as the
form rounds them, to a bound derived from the project's criterion for an fp32-accumulated kernel (tests/sconv_gate_cases.py, parity_excess); AttentionBlock
under set_conv_precision(.., gate="fused"): one gate launch of the form the precision names in place of the library tail, the same calls otherwise, the same
apron, the library path's values to its own tolerance, and the library tail wherever the conditions of the fused one do not hold; whole transforms with the
keyword on, through the entropy codecs."""
import numpy as np
import pytest
import torch

import gpu_support as gs
import sconv_gate_cases as gc
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _name(form):
    return "sconv1x1_gate" + ("" if form == "fp32" else "_" + form)


@pytest.mark.parametrize("name", gc.REAL_CASES)
def test_single_calls_are_held_to_the_bound(lic, name):
    case = gc.BY_NAME[name]
    d = gc.real_data(case)
    dev = {k: gs.dev(v) for k, v in d.items()}
    win = gc.window(case)
    outs = {}
    for form in gc.FORMS:
        sfx = "" if form == "fp32" else "_" + form
        ops = (dev["x"], getattr(lic, "sconv1x1%s_pack" % sfx)(dev["w"]), dev["b"], dev["trunk"], dev["res"])
        got = gs.sentinel_call(lambda out: getattr(lic, _name(form))(*ops, out, ring=case.ring, ring_w=case.ring_w), d["trunk"].shape, gc.SENTINEL)
        want = gc.gate64(d["x"], d["w"], d["b"], d["trunk"], d["res"], form)
        excess = gc.parity_excess(got[win], want[win], d["trunk"][win], d["res"][win])
        print("%s / %s: max |out - ref| %.3g, excess over 1e-4 |trunk| + 1e-6 (1 + |residual|): %.3g" % (name, form, np.abs(got[win] - want[win]).max(), excess))
        assert excess <= 0, (name, form, excess)
        frame = np.ones(got.shape, bool)
        frame[win] = False
        assert (got[frame] == gc.SENTINEL).all()
        outs[form] = got
    assert not np.array_equal(outs["fp32"], outs["bf16x1"])                 # the forms are really distinct


def _gate_calls(calls):
    return {k: v for k, v in calls.made().items() if "_gate" in k}


def _others(calls):
    return {k: v for k, v in calls.counts.items() if "_gate" not in k}


def _block(lm, c=192, seed=21):
    torch.manual_seed(seed)
    return gs.jitter(lm.AttentionBlock(c, 0).to("cuda:0").eval())


def _apron(t):
    m = torch.ones(t.shape[-2:], dtype=torch.bool, device=t.device)
    m[2:-2, 2:-2] = False
    return t[..., m]


@pytest.mark.parametrize("precision", gc.FORMS)
def test_the_block_takes_the_fused_tail(lic, monkeypatch, precision):
    import lic360_models as lm
    from util import _refresh
    gs.count_rule(monkeypatch, lm)
    att = _block(lm)
    x = _refresh(torch.randn((2, 192, 20, 36), device="cuda:0")).contiguous()
    calls = gs.SconvCalls(lic, monkeypatch, gates=True)
    entered = []
    att.attention[3].register_forward_hook(lambda *a: entered.append(1))
    with torch.no_grad():
        never_set = att(x.clone()) if precision == "fp32" else None         # before the attribute was ever set
        lm.set_conv_precision(att, precision)
        calls.reset()
        del entered[:]
        want = att(x.clone())
        lib_counts = dict(_others(calls))
        assert not _gate_calls(calls) and len(entered) == 1 and sum(lib_counts.values()) == 18, calls.counts
        if never_set is not None:
            assert torch.equal(want, never_set)                             # "library" gives the parent's bits
        lm.set_conv_precision(att, precision, gate="fused")
        calls.reset()
        del entered[:]
        xin = x.clone()
        got = att(xin)
        assert _gate_calls(calls) == {_name(precision): 1}, calls.counts   # one launch, of the form the precision names
        assert _others(calls) == lib_counts and not entered
        # the call's own operands through the float64 reference give the block's interior
        _, (a, packed, bias, trunk, residual, out), kw = calls.gates[0]
        assert kw == dict(ring=2) and out.data_ptr() == got.data_ptr() and residual.data_ptr() == xin.data_ptr() and bias.data_ptr() == att.attention[3].bias.data_ptr()
        ops = [t.detach().cpu().numpy() for t in (a, att.attention[3].weight, bias, trunk, residual)]
        ref = gc.gate64(*ops, form=precision)
        inner = (Ellipsis, slice(2, -2), slice(2, -2))
        excess = gc.parity_excess(got.cpu().numpy()[inner], ref[inner], ops[3][inner], ops[4][inner])
        print("%s: excess over the bound %.3g" % (precision, excess))
        assert excess <= 0
        assert torch.equal(_apron(got), _apron(xin)) and torch.equal(_apron(xin), _apron(x))     # x's refreshed apron
        assert torch.equal(_apron(got), _apron(want))
        if precision == "fp32":
            assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())
        assert not torch.equal(got, want)
        # "fused" -> "library" -> "fused": the same bits each way
        lm.set_conv_precision(att, precision)
        assert torch.equal(att(x.clone()), want)
        lm.set_conv_precision(att, precision, gate="fused")
        assert torch.equal(att(x.clone()), got)


def test_the_library_tail_runs_outside_the_conditions(lic, monkeypatch):
    import lic360_models as lm
    from util import _refresh
    gs.count_rule(monkeypatch, lm)
    att = lm.set_conv_precision(_block(lm), "fp32", gate="fused")
    x = _refresh(torch.randn((2, 192, 20, 36), device="cuda:0")).contiguous()
    calls = gs.SconvCalls(lic, monkeypatch, gates=True)
    entered = []
    att.attention[3].register_forward_hook(lambda *a: entered.append(1))

    def library(run):
        calls.reset()
        del entered[:]
        out = run()
        assert not _gate_calls(calls) and len(entered) == 1, calls.counts
        return out

    with torch.no_grad():
        got = att(x.clone())
        assert _gate_calls(calls) == {"sconv1x1_gate": 1} and not entered   # (the conditions hold here)
    # a recorded gradient on x, on every parameter, on one parameter outside the first bottleneck
    library(lambda: att(x.clone().requires_grad_()))
    library(lambda: att(x.clone()))
    for prm in att.parameters():
        prm.requires_grad_(False)
    att.attention[3].bias.requires_grad_(True)
    fused_convs = library(lambda: att(x.clone()))
    assert sum(_others(calls).values()) == 18                               # (the bottlenecks stay fused: only the tail asks for the whole block's parameters)
    att.attention[3].bias.requires_grad_(False)
    calls.reset()
    del entered[:]
    assert torch.equal(att(x.clone()), got) and _gate_calls(calls) == {"sconv1x1_gate": 1} and not entered       # nothing records: fused again, with grad enabled
    assert torch.allclose(fused_convs.detach(), got, rtol=1e-4, atol=1e-4)
    with torch.no_grad():
        # a non-contiguous x
        xt = x.clone().to(memory_format=torch.channels_last)
        assert not xt.is_contiguous()
        out = library(lambda: att(xt))
        assert torch.allclose(out, got, rtol=1e-4, atol=1e-4)
        # a gate convolution without a bias
        bias = att.attention[3].bias
        att.attention[3].bias = None
        library(lambda: att(x.clone()))
        att.attention[3].bias = bias
        # a map that _fusable refuses
        monkeypatch.setattr(lm, "FUSED_MIN_WORKGROUPS", 1 << 30)
        out = library(lambda: att(x.clone()))
        assert sum(calls.counts.values()) == 0 and torch.allclose(out, got, rtol=1e-4, atol=1e-4)
        gs.count_rule(monkeypatch, lm)
        # a 48-channel block
        small = lm.set_conv_precision(_block(lm, 48), "fp32", gate="fused")
        hits = []
        small.attention[3].register_forward_hook(lambda *a: hits.append(1))
        calls.reset()
        small(_refresh(torch.randn((2, 48, 20, 36), device="cuda:0")).contiguous())
        assert not _gate_calls(calls) and len(hits) == 1


def test_whole_transforms_with_the_fused_gate(lic, monkeypatch):
    """image -> analysis -> fused entropy codecs -> bytes -> decode -> synthesis at 192 channels / 48 groups, batch 1, every fused path forced, the fast mode
    with gate="fused": two gate launches per side (the blocks at 132 x 260 and 36 x 68), the latent codes and decodes to the same symbols, the image is finite"""
    import lic360_models as lm
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_main_params, make_imp_params
    gs.count_rule(monkeypatch, lm)
    calls = gs.SconvCalls(lic, monkeypatch, gates=True)
    torch.manual_seed(12)
    C, G = 192, 48
    enc = lm.set_conv_precision(lm.CMP_Encoder(C, C, 8, 0).to("cuda:0").eval(), "bf16x1", stride2="bf16x1", gdn="bf16x3", gate="fused")
    dec = lm.set_conv_precision(lm.CMP_Decoder(C, C, 8, 0).to("cuda:0").eval(), "bf16x1", stride2="bf16x1", gdn="bf16x3", gate="fused")
    with torch.no_grad():
        img = torch.rand((1, 3, 512, 1024), device="cuda:0")
        code, mask, levels = enc(img)
        assert _gate_calls(calls) == {"sconv1x1_gate_bf16x1": 2}, calls.counts
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
        assert _gate_calls(calls) == {"sconv1x1_gate_bf16x1": 2}, calls.counts
        assert tuple(image.shape) == (1, 3, 512, 1024) and bool(torch.isfinite(image).all())
