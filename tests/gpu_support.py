"""What the transforms' GPU tests share, each piece once: the `lic` fixture, host <-> device one-liners, the float64 -> fp32 reference with its cache, the
whole-output and frame comparisons, the sentinel-filled call, the two-stream repeat loop, the past-4 GiB scaffolding, the recorder of lic360.sconv* calls, the
count-rule switch, the block-parameter jitter, the bf16x1 criteria and the canaried allocations (Arena) -- and, for the fused latent codec's tests, the one way to create a codec under its
environment switches (codec_under).  A plain module, imported like util.py and the *_cases.py files; which entry point, pack
and keywords a form takes stays in the form's own test file, which hands a closure `call(out)` to the helpers here.  tests/test_gpu_support_cpu.py checks the
checkers on CPU tensors."""
import functools

import numpy as np
import pytest
import torch

import lic360_models as _lm

COUNT_RULE = ("FUSED_MIN_WORKGROUPS", "FUSED_MIN_FILL", "FUSED_S2_MIN_WORKGROUPS")
_RULE = {name: getattr(_lm, name) for name in COUNT_RULE}                   # lic360_models' own constants, read before any test patches them


@pytest.fixture(scope="module")
def lic():
    """the package, on a machine with a device: a GPU test without one FAILS (a skip would hide a broken run); taken with `from gpu_support import lic`"""
    import lic360
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return lic360


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


# ---- the fused latent codec under its environment switches
# every switch a codec reads when it is created: the names of csrc/codec_switches.h's table, in its order (tests/test_codec_switches_cpu.py compares)
SWITCH_NAMES = ("LIC360_FUSED_CONV", "LIC360_HOST_CODER", "LIC360_NOSKIP", "LIC360_NOCLEAR", "LIC360_DC_NOTALL", "LIC360_DC_ORDER", "LIC360_NOPACK",
                "LIC360_DC_GSTEP", "LIC360_DC_NONETS", "LIC360_EC_GBK", "LIC360_NOBALANCE")


def codec_under(G, H, W, B, layers, **switches):
    """a FusedCodec of max_batch B with the layers loaded, created under exactly the given switches (LIC360_NOSKIP=1, LIC360_DC_ORDER="1p"; None: not
    set) and no other one, whatever the process's environment holds -- which is left as it was"""
    import os
    from lic360_fused import FusedCodec
    assert set(switches) <= set(SWITCH_NAMES), sorted(set(switches) - set(SWITCH_NAMES))
    old = {k: os.environ.pop(k, None) for k in SWITCH_NAMES}
    os.environ.update({k: str(v) for k, v in switches.items() if v is not None})
    try:
        fc = FusedCodec(G, H, W, max_batch=B)
    finally:
        for k in SWITCH_NAMES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    fc.load_layers(layers)
    return fc


# ---- canaried, sentinel-filled, deliberately misaligned allocations (the pointwise / table ops and the fused rate losses)
GUARD_BYTES = 256                # of canary on either side: the carved view keeps the allocation's 256-byte alignment
CANARY = {torch.float32: float(np.float32(-6.0221e23)), torch.float64: -6.0221e23, torch.int64: -0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A}
# what a call leaves unwritten still holds; fp32: the *_cases.py files' UNWRITTEN
SENTINEL = {torch.float32: float(np.float32(7.7701e33)), torch.float64: 7.7701e33, torch.int64: 0x7777777777777777, torch.uint8: 0xA5}


class Arena(object):
    """tensors carved out of canaried allocations; `offset` elements past the aligned start give a 4-byte (odd offset) or 8-byte (offset 2)
    aligned fp32 view that is not 16-byte aligned"""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.bufs = []

    def new(self, shape, offset=0, dtype=torch.float32):
        n = int(np.prod(shape))
        guard = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        buf = torch.full((guard + offset + n + guard,), CANARY[dtype], dtype=dtype, device=self.device)
        view = buf[guard + offset:guard + offset + n].view(*shape)
        view.fill_(SENTINEL[dtype])
        assert view.data_ptr() % 16 == (view.element_size() * offset) % 16 and view.is_contiguous()
        self.bufs.append((buf, guard + offset, n, dtype))
        return view

    def put(self, a, offset=0):
        view = self.new(a.shape, offset)
        view.copy_(torch.from_numpy(np.array(a, copy=True)))
        return view

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        for k, (buf, lo, n, dtype) in enumerate(self.bufs):
            front, back = int((buf[:lo] != CANARY[dtype]).sum()), int((buf[lo + n:] != CANARY[dtype]).sum())
            assert front == 0 and back == 0, "allocation %d: %d canaries overwritten in front, %d behind" % (k, front, back)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(a, b):
    """how many fp32 elements of two arrays of one shape differ in their bits"""
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


_REFS = {}                                                                  # key -> fp32 reference, for the callers that asked to keep it


def fp32_reference(compute, key=None):
    """compute()'s float64 reference as fp32, which it must already be; with a key it is kept (a production case's reference, shared between its exact test and
    its repeat test: the key names the file's form as well, the cache is one per process) and callers leave it unchanged"""
    if key is not None and key in _REFS:
        return _REFS[key]
    want64 = compute()
    want = want64.astype(np.float32)
    assert np.array_equal(want, want64)                                     # the expected values are fp32 numbers
    if key is not None:
        _REFS[key] = want
    return want


def check_whole_output(got, want, describe):
    """window and untouched frame in one comparison: the whole tensor EQUALS the reference (so a NaN fails); describe(got, want) words the failure"""
    assert np.array_equal(got, want), describe(got, want)


def frame_is_untouched(out, r0, r1, c0, c1, sentinel):
    """rows outside r0:r1 and columns outside c0:c1 of a [n, c, rows, cols] array or tensor still hold the sentinel"""
    return bool((out[:, :, :r0] == sentinel).all() and (out[:, :, r1:] == sentinel).all() and
                (out[:, :, :, :c0] == sentinel).all() and (out[:, :, :, c1:] == sentinel).all())


def sentinel_call(call, shape, sentinel):
    """`out` filled with the sentinel, call(out) -- which hands `out` back -- and the host array"""
    out = torch.full(shape, sentinel, device="cuda:0")
    assert call(out) is out
    return host(out)


def repeat_on_two_streams(call, shape, want, sentinel, describe, launches=20):
    """`launches` launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the reference.
    Determinism under ordinary use (two streams, ordinary arguments); stops at the first difference."""
    want_dev = dev(want).float()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty(shape, device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    try:
        for rep in range(0, launches, 2):
            for k, s in enumerate(streams):
                with torch.cuda.stream(s):
                    outs[k].fill_(sentinel)
                    call(outs[k])
            for k, s in enumerate(streams):
                s.synchronize()
                if not torch.equal(outs[k], want_dev):
                    pytest.fail("launch %d (stream %d): %s" % (rep + k, k, describe(host(outs[k]), want)))
    finally:
        torch.cuda.synchronize()


# ---- tensors past 4 GiB: twice the same half-batch of images
def skip_below_free_memory(gib=32):
    free = torch.cuda.mem_get_info()[0]
    if free < gib << 30:
        print("test_past_4gib SKIPPED: %.1f GiB of device memory free, %d needed" % (free / 2.0 ** 30, gib))
        pytest.skip("%.1f GiB of device memory free, %d needed" % (free / 2.0 ** 30, gib))


def doubled(bound, seed, half, shape):
    """[2 half, *shape] of seeded integers in -bound .. bound: image i + half is image i; past 2^33 bytes and 2^31 elements"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    base = torch.randint(-bound, bound + 1, (half,) + tuple(shape), device="cuda:0", generator=g, dtype=torch.float32)
    x = torch.empty((2 * half,) + tuple(shape), device="cuda:0")
    x[:half], x[half:] = base, base
    assert x.numel() * 4 > 2 ** 33 and x.numel() > 2 ** 31
    return x


def pairs_check(out, what):
    """image i equals image i + n / 2, and no two others are equal"""
    half = out.shape[0] // 2
    assert torch.equal(out[:half], out[half:]), "%s: image i and image i + %d differ" % (what, half)
    for i in range(half):
        for j in range(i + 1, half):
            assert not torch.equal(out[i], out[j]), "%s: images %d and %d are equal" % (what, i, j)


# ---- the model-level tests: which entry points a module reaches, and with what
class SconvCalls(object):
    """wraps every callable lic.sconv* that is neither a _pack nor a _supported and counts the calls per name: made() is {name: count} of the names called, so
    a layer that strays to an entry point no test listed shows in it.  By keyword it also keeps `kw`, the (name, form, cpw) of the narrow calls (narrow);
    `gates`, the (name, args, kwargs) of the gate calls (gates); `library`, (cin, cout, ks, stride) of every nn.Conv2d.forward that reaches the library
    (library); `weights`, the weight behind every pack (packs; implied by the next two); while `emulating` is set, x and the weight rounded to bf16 in front of
    the fp32 entry points named by `emulate`; while `recording` is set, `records`: operands (cloned at call time), weight, keywords and output (cloned behind
    the call) of the stride-1 bf16x1 calls (record)."""
    RECORDED = ("sconv3x3_bf16x1", "sconv1x1_bf16x1")

    def __init__(self, lic, monkeypatch, narrow=False, gates=False, library=False, packs=False, emulate=(), record=False):
        self.counts, self.kw, self.gates, self.library, self.records = {}, [], [], [], []
        self.weights, self.rounded_packs = {}, {}                          # pack's data_ptr -> (pack, weight); -> the fp32 pack of the rounded weight
        self.emulating = self.recording = False
        self._keep = dict(narrow=narrow, gates=gates, emulate=tuple(emulate), record=record)
        real = {n: getattr(lic, n) for n in dir(lic) if n.startswith("sconv") and not n.endswith("_supported") and callable(getattr(lic, n))}
        for name, fn in real.items():
            if not name.endswith("_pack"):
                self.counts[name] = 0
                monkeypatch.setattr(lic, name, functools.partial(self._call, fn, name, real.get(name[:8] + "_pack")))   # (the stride-2 forms take the stride-1 pack)
            elif packs or emulate or record:
                monkeypatch.setattr(lic, name, functools.partial(self._pack, fn))
        if library:
            forward = torch.nn.Conv2d.forward

            def conv_forward(mod, x):
                self.library.append((mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0]))
                return forward(mod, x)
            monkeypatch.setattr(torch.nn.Conv2d, "forward", conv_forward)

    def reset(self):
        for k in self.counts:
            self.counts[k] = 0
        for kept in (self.kw, self.gates, self.library, self.records):
            del kept[:]

    def made(self):
        return {k: v for k, v in self.counts.items() if v}

    def only(self, **counts):
        """made() is exactly `counts` (zeros allowed there): the named entry points as often as stated, every other one not at all"""
        return self.made() == {k: v for k, v in counts.items() if v}

    def _pack(self, real, w):
        pk = real(w)
        self.weights[pk.data_ptr()] = (pk, w.detach().clone())
        return pk

    def _call(self, real, name, fp32_pack, *a, **k):
        self.counts[name] += 1
        if self._keep["narrow"] and name.endswith("_narrow"):
            self.kw.append((name, k["form"], k["cpw"]))
        if self._keep["gates"] and "_gate" in name:
            self.gates.append((name, a, k))
        if self.emulating and name in self._keep["emulate"]:
            key = a[1].data_ptr()
            if key not in self.rounded_packs:
                self.rounded_packs[key] = fp32_pack(self.weights[key][1].bfloat16().float())
            return real(a[0].bfloat16().float(), self.rounded_packs[key], *a[2:], **k)
        if self.recording and self._keep["record"] and name in self.RECORDED:
            keep = [None if t is None else t.detach().clone() for t in (a[0],) + tuple(a[2:5])]
            out = real(*a, **k)
            self.records.append((name, keep, self.weights[a[1].data_ptr()][1], dict(k), out.detach().clone()))
            return out
        return real(*a, **k)


def count_rule(monkeypatch, lm, on=True, stride2=False):
    """on: drop lic360_models' count rule (and, when asked, the stride-2 one), so that every layer the kernels take runs fused on a small map;
    off: the module's own constants again"""
    for name in COUNT_RULE[:3 if stride2 else 2]:
        monkeypatch.setattr(lm, name, type(_RULE[name])(0) if on else _RULE[name])
    return lm


def jitter(block):
    """PReLU slopes, biases and GDN parameters (every parameter of at most two dimensions) moved off their symmetric defaults"""
    with torch.no_grad():
        for prm in block.parameters():
            if prm.dim() <= 2:
                prm.add_(0.05 * torch.rand_like(prm))
    return block


# ---- the bf16x1 criteria (tests/test_gpu_sconv_bf16x1.py states where they come from)
def bf16x1_criterion(ref16, ref32, got, window, sentinel, what, frame=True):
    """one call against the float64 convolution of its bf16-rounded operands (1e-4), 16x closer to it than the fp32 convolution is; frame untouched"""
    win = window
    err, gap = float(np.abs(got[win] - ref16[win]).max()), float(np.abs(ref16[win] - ref32[win]).max())
    print("%s: max |got - ref_bf16| = %.3g, max |ref_bf16 - ref_fp32| = %.3g, max |ref_bf16| = %.3g" % (what, err, gap, float(np.abs(ref16[win]).max())))
    assert np.allclose(got[win], ref16[win], rtol=1e-4, atol=1e-4), "%s: max abs error %g" % (what, err)
    assert 16 * err <= gap, "%s: %g from the single-pass bf16 statement, which is only %g from fp32" % (what, err, gap)
    if frame:
        rest = np.ones(got.shape, bool)
        rest[win] = False
        assert np.all(got[rest] == sentinel), what
    return err, gap


def rms(a):
    return float(a.double().pow(2).mean().sqrt())


def bf16x1_ratio(out_b1, out_emu, out_32, what):
    """a chained run in its statistics: rms(bf16x1 - fp32) / rms(emulated - fp32) in [0.9, 1.1]"""
    num, den = rms(out_b1 - out_32), rms(out_emu - out_32)
    print("%s: rms(bf16x1 - fp32) = %.4g, rms(emulated - fp32) = %.4g, ratio %.4f; rms(fp32) = %.4g" % (what, num, den, num / den, rms(out_32)))
    assert den > 0 and 0.9 <= num / den <= 1.1, (what, num, den)
    return num / den
