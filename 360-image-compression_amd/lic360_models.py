"""Analysis / synthesis transforms of the LIC360 codec on this backend: the networks that turn a 512x1024 ERP image
into the (quantised latent, importance mask, importance map) triple the entropy coder consumes, and back.

Architecture and parameter names follow the reference's inference models (test/model_zoo.py:8-205, 334-379) so that its checkpoints
load with `load_state_dict`: the same module tree (`encoder.net.N...`, `decoder.net.N...`, `quant`, `imp`), built here from a few
generic pieces.  When no gradient is recorded, the 3x3 stride-1 convolutions of 96 / 192 channels on maps large enough to fill the chip run
on this package's own kernel (csrc/conv3x3_kernels.hip, `lic360.sconv3x3`): fp32 MFMA, the sphere apron read by index in its tile loader
(no in-place SpherePad in front of it), bias + PReLU + the residual add in its epilogue, the SphereTrim behind it as its output window;
the blocks' 1x1 layers ride on the same body (`lic360.sconv1x1`), and so do the down-sampling layers of the analysis transform: the 3x3
stride-2 convolutions and the 1x1 stride-2 shortcuts of the hidden stages (`lic360.sconv3x3s2` / `sconv1x1s2`, the body's stride-2 forms).
set_conv_precision(model, "bf16x3") moves the stride-1 fused layers to their split-bf16 forms (csrc/sconv_bf16x3.inc), "bf16x1" to their
single-pass bf16 forms (operands rounded once, one MFMA per product), per module.  The stride-2 layers stay fp32 in every such mode unless the
setter's keyword asks otherwise: set_conv_precision(model, precision, stride2="bf16x1") moves them to their own single-pass bf16 forms
(`lic360.sconv3x3s2_bf16x1` / `sconv1x1s2_bf16x1`, csrc/sconv_b1s2.inc), independently of `precision`.
set_conv_precision(model, precision, gate="fused") runs the tail of the attention blocks -- the gate's 1x1 convolution, sigmoid, product and sum -- as one launch
of `lic360.sconv1x1_gate` in the block's precision (csrc/conv3x3_kernels.hip, the gate epilogue); the default, "library", leaves it to torch.
set_conv_precision(model, precision, small="narrow") retries layers whose wide launch would have too few workgroups on narrow ones (`lic360.sconv3x3_narrow` /
`sconv1x1_narrow` / `sconv1x1_gate_narrow`: 96 or 48 output channels per workgroup, the wide kernel's bits).
Routing: which of these forms a layer runs on, or the library, is decided in one function, `_route` -- admission (no recording, GPU fp32, bias, shape), the
precision after the predicates' fallback, the wide launch's count and fill rule, then the narrow retry -- on one statement of the launch geometry (`_workgroups`,
`_fills`).  A block puts its question through `_fusable` / `_fusable_s2`, each layer its own through `_sconv` / `_sconv_gate` / `_sconv_s2`, and `_launch` turns
the answer into the `lic360` call (`_names`: the one place where a function's name is put together).
The first stage's stride-2 layers (3 input channels: no 16-channel chunk, and bound by their output, not by MFMAs), convolutions off the fused
shapes, small maps and every recording (training) pass are library work (torch -> MIOpen); native around them:
sphere pad / trim / cut-edge / pixel-shuffle / importance map / quantiser kernels and the one-pass GDN (csrc/gdn_kernels.hip).
EntropyNet2 is the reference's training-time entropy model of the latent (train/EntropyNet2.py:8-74) on MaskConv2, DropGrad and GmmRateLoss: its
`rate(x, mask)` is the rate term of the training loss, on the fused GMM rate loss with head="fused".
EntropyNet3 is the reference's training-time entropy model of the importance map (test/model_zoo.py:275-300) on MaskConv2, DropGrad and CeRateLoss: its
`rate(x)` is the importance map's rate term, on the fused cross-entropy rate loss with head="fused"."""
import collections
import functools
import types

import torch
from torch import nn
import lic360
from lic360_operator import GDN, Dtow, SpherePad, SphereTrim, SphereCutEdge, QUANT, Dquant, SphereLatScaleNet, ImpMap


def _conv(cin, cout, k, stride=1, pad=0):
    return nn.Conv2d(cin, cout, k, stride, pad)


FUSED_MIN_WORKGROUPS = 256          # lic360.sconv3x3 is used when its workgroups (330 us each) fill whole rounds of the 256 CUs to 80 % or more: 512 per
                                    # 260x516 map -- one image is two exact rounds -- but not 128 (measured against MIOpen, batches 1..8: tools/conv3x3_probe.py)
FUSED_MIN_FILL = 0.8
FUSED_S2_MIN_WORKGROUPS = 128       # lic360.sconv3x3s2 / sconv1x1s2 (one workgroup per 16x16 tile of the OUTPUT window and 192 channels, one workgroup per CU: a round of
                                    # up to 256 takes 0.334 ms at 192 -> 192) are used from this many workgroups on: the smallest count from which they are not slower than
                                    # SpherePad + MIOpen on any measured shape (batches 1..32: tools/conv3x3_probe.py --s2, profiles/sconv_s2_probe.json; at 64 the
                                    # 3x3 loses 1.8x, so SphereConv2 -- 8 tiles per image -- stays on the library below batch 16); past one round the FUSED_MIN_FILL rule holds
SMALL_MODES = ("library", "narrow")
NARROW_CPWS = (96, 48)              # output channels per workgroup of lic360.sconv3x3_narrow / sconv1x1_narrow / sconv1x1_gate_narrow, widest first
NARROW_MIN_WORKGROUPS = 256         # the count rule of the narrow launches is _fusable's (FUSED_MIN_WORKGROUPS, FUSED_MIN_FILL).  A floor of 128 was measured and not taken
                                    # (tools/conv3x3_probe.py --narrow, profiles/sconv_narrow_probe.json; median ms, narrow against library): at batch 1 on 68 x 132 the fp32 3x3
                                    # layers lose at 128 workgroups (cpw 48: V2 conv1 0.137 against 0.092, conv2 0.099 / 0.097, GDN conv2 0.098 / 0.086) while bf16x3 / bf16x1
                                    # win (0.047 / 0.039 against 0.092); the bottleneck at 36 x 68, batch 8, wins in every form (3x3 fp32 0.053 against 0.061).  A per-form floor
                                    # is a lead; one rule for all forms keeps 256.
NARROW_ROUTED_BACK = {("fp32", 3, 96, True)}    # (precision, kernel size, cpw, tall last tile row?) that the count rule admits and the measurement routes back to the
                                    # library: the fp32 3x3 at cpw 96 with a 20-row last tile row -- ResidualBlockV2.conv1 on 132 x 260 at batch 1 -- ran 0.218 ms (0.218 - 0.228)
                                    # against the library's 0.254 (0.252 - 0.290): 0.036 apart, inside the spreads added (0.048).  Without the tall row (conv2, GDN conv2: 0.194 /
                                    # 0.181 against 0.264 / 0.242) and in bf16x3 / bf16x1 (0.072 / 0.045) the same layer passes.  A routed-back layer is not retried narrower
                                    # (cpw 48 there: 0.268); ResidualBlockV2 asks _fusable for its conv1, so in fp32 that block stays on the library at that shape.
CONV_PRECISIONS = ("fp32", "bf16x3", "bf16x1")
STRIDE2_PRECISIONS = ("fp32", "bf16x1")
S2_BF16X1_1X1_MAX_CELLS = 132 * 260  # lic360.sconv1x1s2_bf16x1 is taken on input maps of up to this many cells: the largest on which it beat the fp32 stride-2 kernel by more
                                     # than the repeats' spreads (batch 8: 0.076 against 0.093 ms).  On the 260 x 516 map the shortcut moves 0.8 GB per launch and both forms take
                                     # what the memory takes (0.348 against 0.359 ms, inside the spreads): that shape, and any unmeasured one above the bound, stays on fp32.
                                     # The 3x3 form passed on every production shape (3.7 - 6.4 x) and has no such bound.  tools/conv3x3_probe.py --s2 --precision bf16x1,
                                     # profiles/sconv_s2_bf16x1_probe.json, DESIGN §7c‴.
GDN_PRECISIONS = ("fp32", "bf16x3")
GATE_MODES = ("library", "fused")


def set_conv_precision(module, precision, stride2="fp32", gdn="fp32", gate="library", small="library"):
    """arithmetic of the fused convolutions of every block under `module` (module.modules()): "fp32" (the default: lic360.sconv3x3 / sconv1x1),
    "bf16x3" (their split-bf16 forms wherever those take the layer's shape, the fp32 kernel elsewhere; about 2^-16 relative error per product) or
    "bf16x1" (their single-pass bf16 forms under the same shape rule: every input value and weight rounded once to bf16, one MFMA per product, fp32
    accumulation, bias / PReLU / residual in fp32; about 2^-8 relative per operand -- reduced-precision inference: a latent from any mode codes
    bit-exactly, only decoded pixels depend on the decoder's mode).
    The stride-2 layers do not follow `precision`: in every mode they stay on the fp32 stride-2 kernel (lic360.sconv3x3s2 / sconv1x1s2) unless
    stride2="bf16x1" moves them to their single-pass bf16 forms (lic360.sconv3x3s2_bf16x1 / sconv1x1s2_bf16x1: the bf16x1 contract, wherever those take the
    layer's shape); a later call without the keyword returns them to fp32.
    The GDNs do not follow `precision` either: they stay on the fp32 one-pass kernel (lic360.gdn_forward) unless gdn="bf16x3" moves those of a supported
    channel count to the split-bf16 form (lic360.gdn_bf16x3_forward, csrc/gdn_bf16x3.inc: 2^-15 relative per element against the float64 GDN); a later
    call without the keyword returns them to fp32.
    The gate of the attention blocks -- its 1x1 convolution, the sigmoid, the product with the trunk and the sum with the input -- stays on the library
    (MIOpen / rocBLAS + three elementwise kernels) unless gate="fused" moves it to one launch of lic360.sconv1x1_gate (or its bf16x3 / bf16x1 form, following
    `precision`) wherever the block is on its fused path; a later call without the keyword returns it to "library".
    Layers whose launch would have too few workgroups -- one per 16 x 16 tile and 192 (96) output channels: below FUSED_MIN_WORKGROUPS on a 132 x 260 map at batch 1, on
    36 x 68 maps at batch 8 -- stay on the library unless small="narrow" retries them on narrow workgroups (lic360.sconv3x3_narrow / sconv1x1_narrow /
    sconv1x1_gate_narrow: 96 or 48 output channels per workgroup, the widest whose count passes the same rule; the arithmetic of `precision`, bit for bit the wide
    kernel's result); every other condition of the fused path is unchanged, and a later call without the keyword returns them to the library.
    A per-module setting, not a global: several copies of the networks may run side by side in different modes.  Library layers, small maps and
    recording passes are the same in either mode.  Returns `module`."""
    if precision not in CONV_PRECISIONS:
        raise ValueError("conv precision must be one of %s, got %r" % (CONV_PRECISIONS, precision))
    if stride2 not in STRIDE2_PRECISIONS:
        raise ValueError("stride-2 conv precision must be one of %s, got %r" % (STRIDE2_PRECISIONS, stride2))
    if gdn not in GDN_PRECISIONS:
        raise ValueError("GDN precision must be one of %s, got %r" % (GDN_PRECISIONS, gdn))
    if gate not in GATE_MODES:
        raise ValueError("gate mode must be one of %s, got %r" % (GATE_MODES, gate))
    if small not in SMALL_MODES:
        raise ValueError("small-launch mode must be one of %s, got %r" % (SMALL_MODES, small))
    for m in module.modules():
        m._conv_precision = precision
        m._stride2_precision = stride2
        m._gdn_precision = gdn
        m._gate_mode = gate
        m._small_mode = small
    return module


def set_gdn_grad(module, grad):
    """where the recording passes of every lic360_operator.GDN under `module` go: "library" (the composition and autograd's chain, the default) or "fused"
    (autograd.GdnFn: the one-pass forward and lic360.gdn_backward, which keeps nothing but x).  Returns how many GDNs were set."""
    grad = GDN._grad(grad)
    gdns = [m for m in module.modules() if isinstance(m, GDN)]
    for m in gdns:
        m.grad = grad
    return len(gdns)


def _records_grad(x, conv, mod=None):
    """is a gradient recorded here?  (The kernels have no backward: with gradients enabled a fused path is taken only if neither x, the layer's weight nor ANY parameter
    of the block `mod` that the path pushes through them -- the 1x1 layers, shortcuts, PReLU slopes, biases: all of the block -- requires one)"""
    return torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad or (mod is not None and any(p.requires_grad for p in mod.parameters())))


# The launch geometry, restated from sconv_plan (both strides) and sconv_tall of csrc/conv3x3_kernels.hip (tests/test_sconv_routes_cpu.py holds it against the
# restatements of the exact tests' case files)
def _workgroups(n, nr, nc, cout, ks, stride=1, cpw=None, precision="fp32"):
    """(workgroups, tall last tile row?) of one launch on a window of nr x nc cells -- at stride 2 the OUTPUT's -- of n images: one per 16 x 16 tile and `cpw` output channels,
    on a wide launch the pack's block (192, or all 96); its 8 waves stand NQ = channels / 48 wide, in 8 / NQ row groups.  At stride 1 a 3x3 window's remainder of 1 .. 8 / NQ
    rows rides on the last tile row -- except in bf16x3 at 48 channels per workgroup, whose tall tile does not fit the LDS; any other remainder takes a tile row of its own"""
    nq = cpw // 48 if cpw else 4 if cout % 192 == 0 else 2
    tall = stride == 1 and ks == 3 and not (precision == "bf16x3" and nq == 1) and 0 < nr % 16 <= 8 // nq and nr >= 16
    return n * (nr // 16 if tall else (nr + 15) // 16) * ((nc + 15) // 16) * (cout // cpw if cpw else cout // 192 if nq == 4 else 1), tall


def _fills(workgroups, floor, one_round=False):
    """the count and fill rule: `floor` workgroups or more, in whole rounds of the 256 CUs filled to FUSED_MIN_FILL (300 workgroups would run two rounds for the work of
    1.2) -- with `one_round`, a single round as it is (stride 2: one round of FUSED_S2_MIN_WORKGROUPS or more already wins as measured)"""
    return workgroups >= floor and ((one_round and workgroups <= 256) or workgroups >= FUSED_MIN_FILL * 256 * ((workgroups + 255) // 256))


Route = collections.namedtuple("Route", "ks stride precision cpw gate")      # cpw: output channels per workgroup of a narrow launch, None: the wide kernel


def _route(mod, conv, x, ring=None, ring_w=None, stride=1, ks=None, gate=False, decided=False):
    """THE routing decision of the fused convolutions: the Route on which the layer `conv` (3x3 or 1x1; `gate`: as the attention blocks' gate launch) of block `mod` runs
    on the map x -- at stride 1 on the window inside `ring` rows and `ring_w` columns, at stride 2 (the 3x3 or the 1x1 shortcut of a 2-cell-apron map) on the OUTPUT
    window -- or None: the library.  In this order:
    1. admission: no gradient recorded (_records_grad); a GPU fp32 map, a bias and, at stride 2, a contiguous map; a shape the fp32 form's predicate takes; at stride 2
       an even interior.
    2. precision: the block's (_conv_precision; at stride 2 _stride2_precision, whatever _conv_precision says), unless that form's predicate refuses the shape or the
       measurement sends it back (S2_BF16X1_1X1_MAX_CELLS: the 1x1 stride-2 shortcut on maps above 132 x 260), then fp32.
    3. the wide launch, if its workgroups pass the count and fill rule (_fills: FUSED_MIN_WORKGROUPS, at stride 2 FUSED_S2_MIN_WORKGROUPS with the one-round rule).
    4. only after the wide count has failed, where the block asks for it (set_conv_precision(.., small="narrow"); stride 1; a gate only at cout % 192 == 0): the widest
       cpw of NARROW_CPWS that the narrow form of that precision takes and whose workgroup count -- tiles x cout / cpw, the tall last tile row by the narrow form's own
       rule -- passes the same rule (NARROW_MIN_WORKGROUPS), unless the measurement routed that (precision, ks, cpw, tall) back (NARROW_ROUTED_BACK): a routed-back
       layer is not retried narrower.  A map the wide kernel takes makes no narrow call.
    A block goes one way on this question about ONE of its 3x3 layers (_fusable, _fusable_s2); each of its layers then asks for itself with `decided`, its own kernel
    size and window: admission is behind it and the answer is never None -- a layer no narrow width takes runs wide.  So a sibling whose own narrow count fails where
    the asked layer's passed would run the wide kernel below the count rule; no production block has such a sibling (their layers share one window up to the 1-ring,
    and the counts above are taken per 16-row tile)."""
    ks = conv.kernel_size[0] if ks is None else ks
    cout, cin = conv.weight.shape[:2]
    n, _, hp, wp = x.shape
    if stride == 2:
        nr, nc = (hp - 4) // 2, (wp - 4) // 2
    else:
        ring = (1 if ks == 3 else 2) if ring is None else ring               # (lic360.sconv3x3's / sconv1x1's own default)
        nr, nc = hp - 2 * ring, wp - 2 * (ring if ring_w is None else ring_w)
    if not decided:
        if _records_grad(x, conv, mod):
            return None
        if not (x.is_cuda and x.dtype == torch.float32 and conv.bias is not None and (stride == 1 or x.is_contiguous())):
            return None
        if not _takes(getattr(lic360, _names(ks, "fp32", stride)[2]), cin, cout):
            return None
        if stride == 2 and (hp <= 4 or wp <= 4 or hp % 2 or wp % 2):
            return None
    precision = getattr(mod, "_conv_precision" if stride == 1 else "_stride2_precision", "fp32")
    if precision != "fp32" and not (_takes(getattr(lic360, _names(ks, precision, stride)[2]), cin, cout) and (stride == 1 or ks == 3 or hp * wp <= S2_BF16X1_1X1_MAX_CELLS)):
        precision = "fp32"
    wide = Route(ks, stride, precision, None, gate)
    retry = stride == 1 and getattr(mod, "_small_mode", "library") == "narrow" and nr > 0 and nc > 0 and (not gate or cout % 192 == 0)
    if decided and not retry:
        return wide                                                         # (nothing left to decide: no count is taken)
    if _fills(_workgroups(n, nr, nc, cout, ks, stride)[0], FUSED_MIN_WORKGROUPS if stride == 1 else FUSED_S2_MIN_WORKGROUPS, stride == 2):
        return wide
    if retry:
        for cpw in NARROW_CPWS:
            workgroups, tall = _workgroups(n, nr, nc, cout, ks, 1, cpw, precision)
            if _takes(lic360.sconv_narrow_supported, precision, ks, cin, cout, cpw) and _fills(workgroups, NARROW_MIN_WORKGROUPS):
                if (precision, ks, cpw, tall) in NARROW_ROUTED_BACK:
                    break
                return wide._replace(cpw=cpw)
    return wide if decided else None


@functools.lru_cache(maxsize=1024)
def _takes(predicate, *shape):
    """a shape predicate of lic360 (the attribute as it is at call time), remembered per function and shape: pure, and asked the same few questions on every forward"""
    return bool(predicate(*shape))


@functools.lru_cache(maxsize=None)
def _names(ks, precision, stride=1, narrow=False, gate=False):
    """the names in lic360 of a route's function, of the pack it reads and of its form's shape predicate: the one place where they are put together.  The stride-2 and gate
    forms read the stride-1 pack of their precision (the one the stride-1 form caches); a narrow launch is one function per kernel size, told its form by keyword"""
    size, form = "sconv%dx%d" % (ks, ks), "" if precision == "fp32" else "_" + precision
    kind = size + ("s2" if stride == 2 else "_gate" if gate else "")
    return kind + ("_narrow" if narrow else form), size + form + "_pack", (kind if stride == 2 else size) + form + "_supported"


# (kernel size, precision) -> the names of the convolution, its pack and its shape predicate in lic360.  A bf16x1 row serves every shape its predicate takes:
# each 3x3 and 1x1 shape of the transforms ran faster on it than on bf16x3 by more than the spread of the repeats (DESIGN §7c″, profiles/sconv_bf16x1_probe.json)
_SCONV = {(ks, precision): _names(ks, precision) for ks in (3, 1) for precision in CONV_PRECISIONS}


def _launch(route, conv, x, a, residual, out, **kw):
    """the call a Route stands for (`a`: the PReLU slopes, or the gate's trunk).  The function is lic360's attribute at call time.  The weight travels in the chosen form's
    operand order, repacked when the parameter was written (its version counter) or moved; each precision keeps its own pack, so switching modes never reuses the other's."""
    fn, pack, _ = _names(route.ks, route.precision, route.stride, route.cpw is not None, route.gate)
    if route.cpw is not None:                                               # the same pack on narrow workgroups
        kw.update(form=route.precision, cpw=route.cpw)
    return getattr(lic360, fn)(x, _packed(conv, route.precision, pack), conv.bias, a, residual, out, **kw)


def _packed(conv, precision, pack):
    key = (conv.weight.data_ptr(), conv.weight._version)
    packs = getattr(conv, "_sconv_packs", None)                             # precision -> (key, packed)
    if packs is None:
        packs = conv._sconv_packs = {}
    if packs.get(precision, (None, None))[0] != key:
        packs[precision] = (key, getattr(lic360, pack)(conv.weight.detach()))
    return packs[precision][1]


def _fusable(conv, x, ring, ring_w=None, mod=None):
    """does a block `mod` whose 3x3 stride-1 convolution `conv` meets a map with x's batch, height and width go fused (lic360.sconv3x3, or its narrow form)?"""
    return _route(mod, conv, x, ring, ring_w, ks=3) is not None


def _fusable_s2(conv, x, mod=None):
    """does this stride-2 convolution (3x3 or the 1x1 shortcut) of the 2-cell-apron map x run on lic360.sconv3x3s2 / sconv1x1s2?"""
    return _route(mod, conv, x, stride=2) is not None


def _narrow_cpw(mod, ks, cin, cout, n, nr, nc):
    """the channels per workgroup at which a stride-1 layer (ks x ks, cin -> cout, a window of nr x nc cells on n images) of block `mod` runs on narrow workgroups, or None"""
    layer, window = types.SimpleNamespace(weight=types.SimpleNamespace(shape=(cout, cin, ks, ks))), types.SimpleNamespace(shape=(n, cin, nr, nc))
    return _route(mod, layer, window, 0, ks=ks, decided=True).cpw


def _sconv(mod, conv, x, slope, residual, out, **kw):
    """the fused convolution `conv` (3x3 or 1x1) of block `mod`, in the block's precision and on the workgroups its own window asks for"""
    return _launch(_route(mod, conv, x, kw.get("ring"), kw.get("ring_w"), decided=True), conv, x, slope, residual, out, **kw)


def _sconv_gate(mod, conv, x, trunk, residual, out, **kw):
    """the gate launch of block `mod` on its 1x1 convolution `conv`: lic360.sconv1x1_gate, its bf16x3 / bf16x1 form or the narrow one, under _sconv's rules"""
    return _launch(_route(mod, conv, x, kw.get("ring"), kw.get("ring_w"), ks=1, gate=True, decided=True), conv, x, trunk, residual, out, **kw)


def _sconv_s2(mod, conv, x, slope, residual, out):
    """the stride-2 convolution `conv` (3x3 or the 1x1 shortcut) of block `mod` on a 2-cell-apron map"""
    return _launch(_route(mod, conv, x, stride=2, decided=True), conv, x, slope, residual, out, pad=2, oring=2)


def _scratch(shape, like):
    """an intermediate of a fused block: a fresh buffer per call from the caching allocator (which tracks the stream it is used on), so one model may
    run on several HIP streams at once (module-owned buffers raced there).  Its apron is NOT initialised and need not be: every consumer
    reads aprons by index from the interior (sconv3x3 with sphere != 0), refreshes them in place (SpherePad), works position by position and is trimmed
    afterwards (1x1 layers, PReLU, GDN), or overwrites them (SphereTrim, sphere_apron_from)."""
    return torch.empty(tuple(shape), dtype=torch.float32, device=like.device)


class ResidualBlock(nn.Module):
    """1x1 -> 3x3 -> 1x1 bottleneck on a refreshed apron (model_zoo.py:8-23)"""
    def __init__(self, channels, device_id=0):
        super().__init__()
        half = channels // 2
        self.pad = SpherePad(2, device_id, True)
        self.conv1, self.relu1 = _conv(channels, half, 1), nn.PReLU(half)
        self.conv2, self.relu2 = _conv(half, half, 3, 1, 1), nn.PReLU(half)
        self.conv3 = _conv(half, channels, 1)
        self.trim = SphereTrim(2, device_id)

    def forward(self, x):
        if _fusable(self.conv2, x, 2, mod=self) and x.is_contiguous():
            # conv1 and PReLU are pointwise, so the apron of relu1(conv1(pad(x))) is the sphere wrap of its own interior: conv2 reads it
            # by index and x needs no refresh; only the interior of conv2's output survives the final trim.  The 1x1 layers run on the same
            # kernel body with their PReLU / residual add in the epilogue (interior window only) when their shapes allow it.
            n, c, hp, wp = x.shape
            one = lic360.sconv1x1_supported(c, c // 2) and lic360.sconv1x1_supported(c // 2, c) and self.conv1.bias is not None and self.conv3.bias is not None
            if one:
                y = _scratch((n, c // 2, hp, wp), x)
                _sconv(self, self.conv1, x, self.relu1.weight, None, y, ring=2)
            else:
                y = self.relu1(self.conv1(x)).contiguous()
            y2 = _scratch(y.shape, y)
            _sconv(self, self.conv2, y, self.relu2.weight, None, y2, pad=2, sphere=True, ring=2)
            if one:
                out = torch.empty_like(x)
                _sconv(self, self.conv3, y2, None, x, out, ring=2)
                return self.trim(out)
            return self.trim(x + self.conv3(y2))
        y = self.pad(x)
        y = self.relu2(self.conv2(self.relu1(self.conv1(y))))
        return self.trim(x + self.conv3(y))


class AttentionBlock(nn.Module):
    """x + trunk(x) * sigmoid-gate(x) (model_zoo.py:25-46)"""
    def __init__(self, channels, device_id=0):
        super().__init__()
        three = lambda: [ResidualBlock(channels, device_id) for _ in range(3)]
        self.trunk = nn.Sequential(*three())
        self.attention = nn.Sequential(*three(), _conv(channels, channels, 1), nn.Sigmoid())

    def forward(self, x):
        if _fusable(self.trunk[0].conv2, x, 2, mod=self.trunk[0]):
            fused_tail = getattr(self, "_gate_mode", "library") == "fused" and self._gate_fusable(x)
            x = self.trunk[0].pad(x)                                       # the reference's first ResidualBlock refreshes x's apron in place: `x + ...` below carries it
            if fused_tail:
                # the tail in one launch: out = x + trunk * sigmoid(conv1x1(a) + bias) on the interior.  On the library path trunk(x) is trimmed to zero, so
                # the output's apron is x's refreshed apron: sphere_apron_from writes the same values.
                t, a = self.trunk(x), self.attention[2](self.attention[1](self.attention[0](x)))
                out = torch.empty_like(x)
                _sconv_gate(self, self.attention[3], a, t, x, out, ring=2)
                return lic360.sphere_apron_from(x, out, 2)
        return x + self.trunk(x) * self.attention(x)

    def _gate_fusable(self, x):
        """may the tail run on lic360.sconv1x1_gate?  (behind _fusable of the first bottleneck: a GPU fp32 map large enough, no gradient for x or that block) --
        x contiguous as it arrives (its bottlenecks are then on their fused paths too), no gradient recorded for any parameter of the whole block, a gate
        convolution with a bias and a shape the 1x1 kernel takes"""
        conv = self.attention[3]
        if _records_grad(x, conv, self):
            return False
        cout, cin = conv.weight.shape[:2]
        return x.is_contiguous() and conv.bias is not None and lic360.sconv1x1_supported(cin, cout)


class ResidualBlockV2(nn.Module):
    """two 3x3 convs whose receptive field is fed by the apron (model_zoo.py:48-64)"""
    def __init__(self, channels, device_id):
        super().__init__()
        self.pad = SpherePad(2, device_id, True)
        self.conv1, self.relu1, self.trim1 = _conv(channels, channels, 3, 1, 1), nn.PReLU(channels), SphereTrim(1, device_id)
        self.conv2, self.relu2, self.trim2 = _conv(channels, channels, 3, 1, 1), nn.PReLU(channels), SphereTrim(2, device_id)

    def forward(self, x):
        if _fusable(self.conv1, x, 1, 2, mod=self) and x.is_contiguous():
            # conv1 over the apron read by index, output on the rows of the 1-ring window (the outermost ring is never read) and on the
            # interior's columns only: its input is periodic in longitude, so its 1-ring COLUMNS would repeat its interior's last / first
            # column bit for bit -- conv2 reads them there (longitude wrap), reads the rows as they are, adds x on the interior; the
            # output's apron is x's refreshed apron, as `x + trim2(...)` leaves it in the reference
            y1 = _scratch(x.shape, x)
            _sconv(self, self.conv1, x, self.relu1.weight, None, y1, pad=2, sphere=1, ring=1, ring_w=2)
            out = torch.empty_like(x)
            _sconv(self, self.conv2, y1, self.relu2.weight, x, out, pad=2, sphere=2, ring=2)
            return lic360.sphere_apron_from(x, out, 2)
        y = self.trim1(self.relu1(self.conv1(self.pad(x))))
        return x + self.trim2(self.relu2(self.conv2(y)))


class ResidualBlockDown(nn.Module):
    """stride-2 stage with a GDN branch and a 1x1 stride-2 shortcut; `hidden=False` is the first stage, whose input has no apron yet
    (model_zoo.py:66-95)"""
    def __init__(self, channels, channel_in, device_id, hidden=True):
        super().__init__()
        self.pad1 = SpherePad(2, device_id, hidden)
        self.conv1, self.relu1 = _conv(channel_in, channels, 3, 2, 3), nn.PReLU(channels)
        self.trim = SphereTrim(2, device_id)
        self.pad2 = SpherePad(2, device_id, True)
        self.conv2, self.relu2 = _conv(channels, channels, 3, 1, 1), GDN(channels, device_id)
        self.short_cut = _conv(channel_in, channels, 1, 2, 2)
        self.hidden = hidden

    def forward(self, x):
        if self.hidden and _fusable_s2(self.conv1, x, self) and _fusable_s2(self.short_cut, x, self):
            n, _, hp, wp = x.shape
            shape = (n, self.conv1.out_channels, (hp - 4) // 2 + 4, (wp - 4) // 2 + 4)
            y = _scratch(shape, x)
            if _fusable(self.conv2, y, 2, mod=self):                        # (the whole block goes one way: FUSED_MIN_WORKGROUPS rules its stride-2 layers too)
                # conv1 reads x's apron by index (no pad1: x is not modified), conv2 reads conv1's likewise, GDN is pointwise, the shortcut reads the interior
                # only and adds the GDN output in its epilogue; every apron cell on the way is scratch, the final trim zeroes the output's
                _sconv_s2(self, self.conv1, x, self.relu1.weight, None, y)
                y = self.relu2(_sconv(self, self.conv2, y, None, None, _scratch(shape, x), pad=2, sphere=True, ring=2))
                return self.trim(_sconv_s2(self, self.short_cut, x, None, y, _scratch(shape, x)))
        if self.hidden:
            skip = self.short_cut(x)                                        # before pad1 refreshes the apron in place
            y = self.pad1(x)
        else:
            x = self.pad1(x)
            skip, y = None, x
        # (the reference trims here and refreshes the same apron at once -- `trim` then `pad2` in place, model_zoo.py:83-84,90-91: the refresh
        #  overwrites every cell the trim zeroed, and the fused conv2 does not read the apron at all: one launch less on either path, same result)
        y = self.relu1(self.conv1(y))
        if torch.is_grad_enabled() and y.requires_grad:
            y = self.trim(y)                                                # a recording pass keeps the reference's sequence: the in-place pad's backward leaves the apron's gradient for the trim's to zero
        if _fusable(self.conv2, y, 2, mod=self) and y.is_contiguous():
            # conv2 reads the apron of y by index (no pad2); GDN is pointwise over positions, its frame cells are trimmed below
            y2 = _scratch(y.shape, y)
            y = self.relu2(_sconv(self, self.conv2, y, None, None, y2, pad=2, sphere=True, ring=2))
        else:
            y = self.relu2(self.conv2(self.pad2(y)))
        return self.trim((self.short_cut(x) if skip is None else skip) + y)


class SphereConv2(nn.Module):
    def __init__(self, channel_in, channel_out, kernel_size, stride, pad=0, device_id=0):
        super().__init__()
        self.conv = _conv(channel_in, channel_out, kernel_size, stride, pad)
        self.pad, self.trim = SpherePad(2, device_id, True), SphereTrim(2, device_id)

    def forward(self, x):
        c = self.conv
        if (c.kernel_size, c.stride, c.padding) == ((3, 3), (2, 2), (3, 3)) and type(self) is SphereConv2 and _fusable_s2(c, x, self):
            return _sconv_s2(self, c, x, None, None, None)                        # pad, convolution and trim: the interior window of a zero-filled map
        return self.trim(self.conv(self.pad(x)))


class SphereConv3(SphereConv2):
    """the same with an out-of-place pad: the synthesis side's first layer, whose input has no apron (model_zoo.py:158-168)"""
    def __init__(self, channel_in, channel_out, kernel_size, stride, pad=0, device_id=0):
        super().__init__(channel_in, channel_out, kernel_size, stride, pad, device_id)
        self.pad = SpherePad(2, device_id, False)


class EncoderV2(nn.Module):
    """image [n,3,512,1024] -> (code in (0,1) [n,cc,32,64], importance map [n,1,32,64]); every map carries a 2-cell sphere apron
    until the final cut (model_zoo.py:108-143)"""
    def __init__(self, channels, code_channels, device_id):
        super().__init__()
        d = device_id
        self.net = nn.Sequential(ResidualBlockDown(channels, 3, d, False), ResidualBlockV2(channels, d), ResidualBlockDown(channels, channels, d),
                                 AttentionBlock(channels, d), ResidualBlockV2(channels, d), ResidualBlockDown(channels, channels, d),
                                 ResidualBlockV2(channels, d), SphereConv2(channels, channels, 3, 2, 3, d))
        self.net2 = nn.Sequential(AttentionBlock(channels, d), _conv(channels, code_channels, 1), SphereCutEdge(2, d), nn.Sigmoid())
        self.imp_net = nn.Sequential(ResidualBlockV2(channels, d), ResidualBlockV2(channels, d), _conv(channels, 1, 1), nn.Sigmoid(),
                                     SphereCutEdge(2, d), SphereLatScaleNet(512 // 16, d))
        self.imp_net[2].bias.data.fill_(3)

    def forward(self, x):
        t = self.net(x)
        return self.net2(t), self.imp_net(t)


class ResidualBlockUp(nn.Module):
    """x2 upsampling stage: conv to 4c + pixel shuffle, an inverse-GDN branch, a 1x1 shortcut through its own shuffle (model_zoo.py:145-170)"""
    def __init__(self, channels, device_id):
        super().__init__()
        d = device_id
        self.pad1 = SpherePad(2, d, True)
        self.conv1, self.relu1 = _conv(channels, channels * 4, 3, 1), nn.PReLU(channels * 4)
        self.dtow1, self.trim1 = Dtow(2, True, d), SphereTrim(2, d)
        self.pad2 = SpherePad(2, d, True)
        self.conv2, self.relu2 = _conv(channels, channels, 3, 1, 1), GDN(channels, d, inverse=True)
        self.short_cut = _conv(channels, channels * 4, 1)
        self.cut_edge, self.dtow2, self.trim2 = SphereCutEdge(1, d), Dtow(2, True, d), SphereTrim(2, d)

    def forward(self, x):
        if _fusable(self.conv1, x, 2, mod=self) and x.is_contiguous():
            # the unpadded conv1 (output (h+2) x (w+2)) with PReLU in its epilogue, on the INTERIOR's window only: its 1-ring outputs become the
            # 2-ring of the shuffled map, which trim1 zeroes; x's apron is read by index (no pad1), and the shortcut's apron cells end in the
            # rings trim2 zeroes
            # ... and the pixel shuffle is the kernel's store pattern (a lane's four accumulator registers are one 2 x 2 block of the shuffled
            # map): conv1 -> PReLU -> Dtow -> trim1 in one launch.  The window lands exactly on the shuffled map's interior; its apron is
            # never read (conv2 reads aprons by index, or pad2 refreshes it), so trim1 has nothing to do.
            n, c, hp, wp = x.shape
            b = _scratch((n, self.conv1.out_channels // 4, 2 * (hp - 2), 2 * (wp - 2)), x)
            _sconv(self, self.conv1, x, self.relu1.weight, None, b, pad=2, sphere=1, ring=2, crop=1, shuffle=True)
        else:
            b = self.dtow1(self.relu1(self.conv1(self.pad1(x))))           # (trim1 -> pad2 in place, model_zoo.py:160-161: the refresh overwrites what the trim zeroed)
            if torch.is_grad_enabled() and b.requires_grad:
                b = self.trim1(b)                                           # (recording pass: the reference's sequence, see ResidualBlockDown)
        fused2 = _fusable(self.conv2, b, 2, mod=self)                       # (asked once: relu2 keeps the map's shape, and only parameters of this block, which the question covers, could make its output record)
        if fused2 and b.is_contiguous():
            b2 = _scratch(b.shape, b)
            b = self.relu2(_sconv(self, self.conv2, b, None, None, b2, pad=2, sphere=True, ring=2))
        else:
            b = self.relu2(self.conv2(self.pad2(b)))
        c_in, c_out = self.short_cut.in_channels, self.short_cut.out_channels
        if (fused2 and x.is_contiguous() and b.is_contiguous() and lic360.sconv1x1_supported(c_in, c_out) and self.short_cut.bias is not None
                and tuple(b.shape) == (x.shape[0], c_out // 4, 2 * (x.shape[2] - 2), 2 * (x.shape[3] - 2))):
            # the shortcut -- cut_edge(1) -> 1x1 conv to 4c -> Dtow(2) -- and the `b +` in one launch: the 1x1 instantiation with the shuffled store,
            # b as its (shuffled) residual, on the interior window (trim2 zeroes the rest)
            out = torch.empty_like(b)
            _sconv(self, self.short_cut, x, None, b, out, ring=2, crop=1, shuffle=True)
            return self.trim2(out)
        return self.trim2(b + self.dtow2(self.short_cut(self.cut_edge(x))))


class Decoder(nn.Module):
    """latent [n,cc,32,64] -> image [n,3,512,1024] (model_zoo.py:172-205)"""
    def __init__(self, channels, code_channels, device_id):
        super().__init__()
        d = device_id
        self.net = nn.Sequential(SphereConv3(code_channels, channels, 1, 1, 0, d), AttentionBlock(channels, d), ResidualBlockV2(channels, d),
                                 ResidualBlockUp(channels, d), ResidualBlockV2(channels, d), ResidualBlockUp(channels, d), AttentionBlock(channels, d),
                                 ResidualBlockV2(channels, d), ResidualBlockUp(channels, d), ResidualBlockV2(channels, d), SpherePad(2, d, True),
                                 _conv(channels, 12, 3, 1, 1), SphereCutEdge(2, d), Dtow(2, True, d))

    def forward(self, x):
        return self.net(x)


class CMP_Encoder(nn.Module):
    """image -> (symbols 0..7 under the mask [n,48,64,128], mask [n,48,64,128], importance levels [n,1,32,64]): what EntEncoderFast /
    FusedCodec.encode and ImpEntEncoderFast / FusedImpCodec.encode take (model_zoo.py:334-356)"""
    def __init__(self, channels=192, code_channels=192, quant_levels=8, gpu_id=0):
        super().__init__()
        self.encoder = EncoderV2(channels, code_channels, gpu_id)
        self.imp_level = code_channels // 4
        self.quant = QUANT(code_channels, quant_levels, device_id=gpu_id, ntop=2)
        self.imp = ImpMap(1, 0.0001, 0.0001, self.imp_level, 0.618, 0.618, 3, gpu_id, 2)
        self.dtw1, self.dtw2 = Dtow(2, True, gpu_id), Dtow(2, True, gpu_id)

    def forward(self, x):
        code, imap = self.encoder(x)
        tcode, mask, _ = self.imp(code, imap)
        _, qy = self.quant(tcode)
        return self.dtw1(qy), self.dtw2(mask), torch.sum(mask, dim=1, keepdim=True) / 4


class CMP_Decoder(nn.Module):
    """(symbols, mask) as decoded from the bitstreams -> image (model_zoo.py:358-379)"""
    def __init__(self, channels=192, code_channels=192, quant_levels=8, gpu_id=0):
        super().__init__()
        self.decoder = Decoder(channels, code_channels, gpu_id)
        self.imp_level = code_channels // 4
        self.quant = Dquant(code_channels, quant_levels, device=gpu_id)
        self.dtw1, self.dtw2 = Dtow(2, False, gpu_id), Dtow(2, False, gpu_id)

    def forward(self, code, mask):
        return self.decoder(self.quant(self.dtw1(code), self.dtw2(mask)))


class EntropyResidualBlock(nn.Module):
    """two hidden group-causal 5x5 convolutions with PReLU around a skip (train/EntropyNet2.py:8-21); conv: the route of both MaskConv2"""
    def __init__(self, ngroups, cpn, device_id=0, conv="library"):
        super().__init__()
        from lic360_operator import MaskConv2
        self.net = nn.Sequential(MaskConv2(ngroups, cpn, cpn, 5, True, device_id, route=conv), nn.PReLU(ngroups * cpn),
                                 MaskConv2(ngroups, cpn, cpn, 5, True, device_id, route=conv), nn.PReLU(ngroups * cpn))

    def forward(self, x):
        return self.net(x) + x


class EntropyNet2(nn.Module):
    """The training-time entropy model of the latent (reference train/EntropyNet2.py:24-74): three group-causal nets give every symbol the
    logits, sigmas and means of a `num_gaussian`-component mixture.  Same submodule and parameter names (`weight_net.N...`, `delta_net.N...`,
    `mean_net.N...`), so lic360_codec.cast_entropy_parameter maps its state_dict (under `ent.`) onto the codec drivers; the last sigma layer's
    bias starts at 2.  The parameter-free tail of the reference's nets (ContextReshape, Softmax, ReLU) lives in GmmRateLoss.
    forward(x) -> the reference's per-symbol loss_vec [n * ngroups * h * w], always on the library composition.
    rate(x, mask=None) -> GmmRateLoss's (nats [n] float64, symbols [n] int64) on the route `head` names ("library" or "fused").
    conv: the route of every MaskConv2 ("library" or "fused": the native forward and backward of the group-causal convolution)."""
    def __init__(self, ngroups, cpn=4, num_gaussian=3, device_id=0, drop_flag=False, head="library", conv="library"):
        super().__init__()
        from lic360_operator import MaskConv2, DropGrad, GmmRateLoss
        self.drop = DropGrad(drop_flag)

        def net():
            return nn.Sequential(MaskConv2(ngroups, 1, cpn, 5, False, device_id, route=conv), nn.PReLU(ngroups * cpn),
                                 *[EntropyResidualBlock(ngroups, cpn, device_id, conv) for _ in range(5)],
                                 MaskConv2(ngroups, cpn, num_gaussian, 5, True, device_id, route=conv))
        self.weight_net, self.mean_net, self.delta_net = net(), net(), net()
        self.delta_net[7].bias.data.fill_(2)
        self.head = GmmRateLoss(ngroups, num_gaussian, head, device_id)

    def _nets(self, x):
        tx = self.drop(x)
        return self.weight_net(tx), self.delta_net(tx), self.mean_net(tx), tx

    def forward(self, x):
        logit, sigma, mean, tx = self._nets(x)
        return self.head.loss_vec(logit, sigma, mean, tx)

    def rate(self, x, mask=None):
        logit, sigma, mean, tx = self._nets(x)
        return self.head(logit, sigma, mean, tx, mask)


class EntropyNet3(nn.Module):
    """The training-time entropy model of the importance map (reference test/model_zoo.py:275-300): one group-causal net gives every symbol
    nvalue + 1 logits.  Same submodule and parameter names (`net.N...`), so lic360_codec.cast_imp_entropy_parameter maps its state_dict (under
    `imp_ent.`) onto the importance-map drivers; the gradient stops at the input (DropGrad(True)), which the net sees as x / ((nvalue - 1) / 2) - 1.
    The parameter-free tail of the reference's net (ContextReshape) and its CrossEntropyLoss live in CeRateLoss.
    forward(x) -> the reference's per-symbol loss_vec [n * ngroups * h * w], always on the library composition.
    rate(x) -> CeRateLoss's (nats [n] float64, symbols [n] int64) on the route `head` names ("library" or "fused").
    conv: the route of every MaskConv2 ("library" or "fused"); under "fused" the first layer's data gradient is never computed (its input needs none)."""
    def __init__(self, ngroups, cpn, nvalue=48, device_id=0, head="library", conv="library"):
        super().__init__()
        from lic360_operator import MaskConv2, DropGrad, CeRateLoss
        self.drop = DropGrad(True)
        self.net = nn.Sequential(MaskConv2(ngroups, 1, cpn, 5, False, device_id, route=conv), nn.PReLU(ngroups * cpn),
                                 *[EntropyResidualBlock(ngroups, cpn, device_id, conv) for _ in range(5)],
                                 MaskConv2(ngroups, cpn, nvalue + 1, 5, True, device_id, route=conv))
        self.scale = (nvalue - 1.) / 2.
        self.head = CeRateLoss(ngroups, nvalue + 1, head, device_id)

    def _net(self, x):
        x = self.drop(x)
        return self.net(x / self.scale - 1.), x

    def forward(self, x):
        logit, label = self._net(x)
        return self.head.loss_vec(logit, label)

    def rate(self, x):
        logit, label = self._net(x)
        return self.head(logit, label)


def transform_gflops(channels=192, code_channels=192, h=512, w=1024):
    """nominal conv + GDN GFLOP of one analysis and one synthesis pass (2 flops per MAC; aprons counted: every map is 4 cells larger)"""
    def conv(cin, cout, k, hh, ww):
        return 2.0 * cin * cout * k * k * hh * ww
    c, enc, dec = channels, 0.0, 0.0
    bott = lambda hh, ww: conv(c, c // 2, 1, hh, ww) + conv(c // 2, c // 2, 3, hh, ww) + conv(c // 2, c, 1, hh, ww)
    att = lambda hh, ww: 6 * bott(hh, ww) + conv(c, c, 1, hh, ww)
    v2 = lambda hh, ww: 2 * conv(c, c, 3, hh, ww)
    hh, ww, cin = h, w, 3
    for stage in range(3):                                                  # three down stages
        hh, ww = hh // 2 + 4, ww // 2 + 4
        enc += conv(cin, c, 3, hh, ww) + conv(c, c, 3, hh, ww) + conv(c, c, 1, hh, ww) + conv(cin, c, 1, hh, ww) + v2(hh, ww)
        if stage == 1:
            enc += att(hh, ww)
        cin = c
        hh, ww = hh - 4, ww - 4
    hh, ww = hh // 2 + 4, ww // 2 + 4                                       # 36 x 68
    enc += conv(c, c, 3, hh, ww) + att(hh, ww) + conv(c, code_channels, 1, hh, ww) + 2 * v2(hh, ww) + conv(c, 1, 1, hh, ww)
    dec += conv(code_channels, c, 1, hh, ww) + att(hh, ww) + v2(hh, ww)
    for stage in range(3):                                                  # three up stages
        dec += conv(c, 4 * c, 3, hh, ww) + conv(c, 4 * c, 1, hh, ww)
        hh, ww = (hh - 4) * 2 + 4, (ww - 4) * 2 + 4
        dec += conv(c, c, 3, hh, ww) + conv(c, c, 1, hh, ww) + v2(hh, ww)
        if stage == 1:
            dec += att(hh, ww)
    dec += conv(c, 12, 3, hh, ww)
    return enc / 1e9, dec / 1e9
