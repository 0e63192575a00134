"""The checkers of tests/gpu_support.py on CPU tensors of a few dozen elements: each of them FAILS on the fault it exists to find.  A shared checker that
has gone blind hides every failure behind it.  (sentinel_call and the two-stream loop need a device: the GPU suite runs them.)"""
import types

import numpy as np
import pytest
import torch

import gpu_support as gs

S = 7.0


def _out():
    """[1, 2, 6, 8] with a 2-cell frame of the sentinel around a 2 x 4 window of small integers"""
    out = np.full((1, 2, 6, 8), S, np.float32)
    out[:, :, 2:4, 2:6] = np.arange(16, dtype=np.float32).reshape(1, 2, 2, 4)
    return out


def _describe(got, want):
    return "%d cells differ" % int((got != want).sum())


@pytest.mark.parametrize("cell,value", [((0, 1, 3, 4), 99.0), ((0, 0, 1, 3), 0.0), ((0, 1, 2, 2), np.nan)], ids=["window", "frame", "nan"])
def test_check_whole_output_fails_on_one_cell(cell, value):
    want = _out()
    gs.check_whole_output(want.copy(), want, _describe)
    got = want.copy()
    got[cell] = value
    with pytest.raises(AssertionError, match="1 cells differ"):
        gs.check_whole_output(got, want, _describe)


@pytest.mark.parametrize("cell", [(0, 0, 1, 4), (0, 1, 4, 4), (0, 0, 3, 1), (0, 1, 3, 6)], ids=["top", "bottom", "left", "right"])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_frame_is_untouched_sees_each_side(cell, as_tensor):
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    out = _out()
    assert gs.frame_is_untouched(conv(out), 2, 4, 2, 6, S)
    out[cell] = 0.0
    assert not gs.frame_is_untouched(conv(out), 2, 4, 2, 6, S)


def test_fp32_reference_refuses_what_is_not_an_fp32_number():
    exact = np.array([1.0, 2.0 ** 24, -0.5])
    assert gs.fp32_reference(lambda: exact).dtype == np.float32
    with pytest.raises(AssertionError):
        gs.fp32_reference(lambda: np.array([1.0, 2.0 ** 24 + 1]))
    calls = []
    first = gs.fp32_reference(lambda: (calls.append(1), exact)[1], key=("self-test", 1))
    assert gs.fp32_reference(lambda: (calls.append(1), exact)[1], key=("self-test", 1)) is first and calls == [1]     # kept per key


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int64, torch.uint8], ids=str)
def test_arena_catches_an_overwritten_canary_on_either_side(dtype):
    ar = gs.Arena(device="cpu")
    first, view = ar.new((2, 3), dtype=dtype), ar.new((3, 5), offset=1, dtype=dtype)
    assert (view == gs.SENTINEL[dtype]).all() and view.device.type == "cpu" and view.data_ptr() % 16 == view.element_size() % 16
    view.zero_()                                                            # a call that writes its whole output and nothing else
    first[0, 0] = 1
    ar.check()
    buf, lo, n, _ = ar.bufs[1]
    assert buf[lo:lo + n].data_ptr() == view.data_ptr() and lo * view.element_size() == gs.GUARD_BYTES + view.element_size()
    for where, said in ((lo - 1, "allocation 1: 1 canaries overwritten in front, 0 behind"), (lo + n, "allocation 1: 0 canaries overwritten in front, 1 behind")):
        kept = buf[where].clone()
        buf[where] = 0
        with pytest.raises(AssertionError, match=said):
            ar.check()
        buf[where] = kept
    ar.check()
    if dtype == torch.float32:
        put = ar.put(np.arange(6, dtype=np.float32).reshape(2, 3), offset=2)
        assert put.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]] and put.data_ptr() % 16 == 8
        ar.check()


def test_same_bits_and_differing_compare_bits_not_values():
    a = np.array([0.0, 1.0, np.nan], np.float32)
    assert gs.same_bits(a, a.copy()) and gs.differing(a, a.copy()) == 0     # a NaN equals itself bit for bit
    b = a.copy()
    b[0] = -0.0                                                             # equal as a value, another bit pattern
    assert not gs.same_bits(a, b) and gs.differing(a, b) == 1
    assert not gs.same_bits(a, a.reshape(3, 1))


def test_bf16x1_criterion():
    win = (slice(None), slice(None), slice(2, 4), slice(2, 6))
    ref16 = _out().astype(np.float64)
    ref32 = ref16.copy()
    ref32[win] += 1e-3                                                      # fp32 lies 1e-3 from the bf16 statement: 16x closer is 6.25e-5
    assert gs.bf16x1_criterion(ref16, ref32, ref16.astype(np.float32), win, S, "exact") == (0.0, pytest.approx(1e-3))
    far = ref16.copy()
    far[0, 1, 3, 4] += 1e-2                                                 # beyond 1e-4 (of 12)
    with pytest.raises(AssertionError, match="max abs error"):
        gs.bf16x1_criterion(ref16, ref32, far, win, S, "far")
    near = ref16.copy()
    near[0, 0, 2, 2] += 9e-5                                                # within 1e-4, but not 16x closer to ref16 than ref32 is
    with pytest.raises(AssertionError, match="from the single-pass bf16 statement"):
        gs.bf16x1_criterion(ref16, ref32, near, win, S, "near")
    touched = ref16.copy()
    touched[0, 0, 0, 0] = 0.0
    with pytest.raises(AssertionError, match="^touched"):
        gs.bf16x1_criterion(ref16, ref32, touched, win, S, "touched")
    gs.bf16x1_criterion(ref16, ref32, touched, win, S, "touched, frame not asked", frame=False)


def _fake_lic():
    seen = []

    def conv(x, packed, *a, **k):
        seen.append((x.clone(), packed.clone()))
        return x
    fns = {name: conv for name in ("sconv3x3", "sconv1x1", "sconv3x3s2", "sconv3x3_bf16x1", "sconv1x1_gate_narrow", "sconv9x9_of_tomorrow")}
    fns.update({name: (lambda w: w.clone()) for name in ("sconv3x3_pack", "sconv1x1_pack", "sconv3x3_bf16x1_pack")})
    fns.update({name: (lambda *a: True) for name in ("sconv3x3_supported", "sconv_narrow_supported")})
    return types.SimpleNamespace(SENTINEL=S, sconv_version="not callable", gdn_forward=conv, **fns), seen


def test_sconv_calls_counts_every_convolution_and_nothing_else(monkeypatch):
    lic, _ = _fake_lic()
    calls = gs.SconvCalls(lic, monkeypatch, narrow=True, gates=True)
    assert set(calls.counts) == {"sconv3x3", "sconv1x1", "sconv3x3s2", "sconv3x3_bf16x1", "sconv1x1_gate_narrow", "sconv9x9_of_tomorrow"} and not calls.made()
    x = torch.ones(3)
    w = lic.sconv3x3_pack(x)
    assert lic.sconv3x3_supported(1, 2) and lic.sconv_narrow_supported("fp32", 3, 1, 2, 48) and not calls.made() and not calls.weights
    lic.sconv3x3(x, w)
    lic.sconv3x3(x, w)
    lic.sconv9x9_of_tomorrow(x, w)                                          # an entry point no test lists
    lic.sconv1x1_gate_narrow(x, w, form="bf16x1", cpw=48)
    lic.gdn_forward(x, w)
    assert calls.made() == dict(sconv3x3=2, sconv9x9_of_tomorrow=1, sconv1x1_gate_narrow=1)
    assert not calls.only(sconv3x3=2, sconv1x1_gate_narrow=1) and calls.only(sconv3x3=2, sconv9x9_of_tomorrow=1, sconv1x1_gate_narrow=1, sconv1x1=0)
    assert calls.kw == [("sconv1x1_gate_narrow", "bf16x1", 48)] and [g[0] for g in calls.gates] == ["sconv1x1_gate_narrow"]
    calls.reset()
    assert not calls.made() and not any(calls.counts.values()) and not calls.kw and not calls.gates


def test_sconv_calls_emulate_rounds_x_and_the_weight(monkeypatch):
    lic, seen = _fake_lic()
    calls = gs.SconvCalls(lic, monkeypatch, emulate=("sconv3x3", "sconv3x3s2"), record=True)
    x, w = torch.tensor([1.0, 1.0 + 2.0 ** -10, 3.0]), torch.tensor([257.0, 0.1])
    assert x.bfloat16().float().tolist() != x.tolist() and w.bfloat16().float().tolist() != w.tolist()
    pk = lic.sconv3x3_pack(w)
    assert torch.equal(calls.weights[pk.data_ptr()][1], w)
    lic.sconv3x3(x, pk)                                                     # not emulating: the operands as they are
    calls.emulating = True
    lic.sconv3x3(x, pk)
    lic.sconv3x3s2(x, pk)                                                   # the stride-2 form reads the stride-1 pack
    lic.sconv1x1(x, pk)                                                     # not named by `emulate`
    calls.emulating, calls.recording = False, True
    lic.sconv3x3_bf16x1(x, pk, None, None, None, a=1)
    rounded = (x.bfloat16().float(), w.bfloat16().float())
    for (gx, gw), (wx, ww) in zip(seen, [(x, w), rounded, rounded, (x, w), (x, w)]):
        assert torch.equal(gx, wx) and torch.equal(gw, ww)
    assert len(seen) == 5 and calls.made() == dict(sconv3x3=2, sconv3x3s2=1, sconv1x1=1, sconv3x3_bf16x1=1)
    (name, keep, weight, kw, out), = calls.records
    assert name == "sconv3x3_bf16x1" and torch.equal(keep[0], x) and keep[1:] == [None, None, None] and torch.equal(weight, w) and kw == dict(a=1)


def test_count_rule_drops_and_restores_the_modules_own_constants(monkeypatch):
    import lic360_models as lm
    own = {name: getattr(lm, name) for name in gs.COUNT_RULE}
    assert own["FUSED_MIN_WORKGROUPS"] > 0 and own["FUSED_MIN_FILL"] > 0 and own["FUSED_S2_MIN_WORKGROUPS"] > 0
    assert gs.count_rule(monkeypatch, lm) is lm
    assert (lm.FUSED_MIN_WORKGROUPS, lm.FUSED_MIN_FILL, lm.FUSED_S2_MIN_WORKGROUPS) == (0, 0.0, own["FUSED_S2_MIN_WORKGROUPS"])
    gs.count_rule(monkeypatch, lm, stride2=True)
    assert lm.FUSED_S2_MIN_WORKGROUPS == 0
    monkeypatch.setattr(lm, "FUSED_MIN_WORKGROUPS", 1 << 30)               # whatever a test left there
    gs.count_rule(monkeypatch, lm, on=False, stride2=True)
    assert {name: getattr(lm, name) for name in gs.COUNT_RULE} == own


def test_jitter_moves_the_small_parameters_only():
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(2, 2, 3)
    w, b = conv.weight.detach().clone(), conv.bias.detach().clone()
    assert gs.jitter(conv) is conv
    assert torch.equal(conv.weight, w) and bool((conv.bias > b).all()) and bool((conv.bias <= b + 0.05).all())
