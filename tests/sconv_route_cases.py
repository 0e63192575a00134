"""The routes lic360_models takes through the fused sphere convolutions, tabulated: which `lic360.sconv*` function a layer of a block runs on, in which form and at
how many channels per workgroup, over the production layer signatures x maps x batches x precisions x small-launch modes.  No GPU: the decision is shape arithmetic
plus the library's shape predicates, which load on a CPU-only machine.  Only the seam of lic360_models is driven -- _fusable / _fusable_s2 for the block's question,
_sconv / _sconv_gate / _sconv_s2 for the layer's call -- on a fake map, with every public `lic360.sconv*` call replaced by a recorder and `_packed` stubbed, so the
same enumeration runs on any version of that file.  tests/test_sconv_routes_cpu.py compares it with the committed table tests/golden/sconv_routes.json.

A table row is one (layer, map, mode); its value holds one token per batch of BATCHES: the block's answer about this layer (y / n; `.` where no block asks about
such a layer), the function called without its `sconv` prefix, `:form:cpw` of a narrow call, `@` the precision whose pack it was handed.  The call is recorded
whatever the answer: a block goes one way on the question about one of its 3x3 layers, and its other layers then launch without asking again.

    python tests/sconv_route_cases.py path/to/lic360_models.py > tests/golden/sconv_routes.json     # the table of that version of the file"""
import collections
import importlib.util
import json
import os
import sys

import torch

MAPS = ((36, 68), (68, 132), (132, 260), (260, 516), (516, 1028))
BATCHES = (1, 2, 4, 8, 16, 32)

Layer = collections.namedtuple("Layer", "name cin cout ks kw")
# the stride-1 calls of the production blocks (ResidualBlock's three layers, ResidualBlockV2.conv1 and .conv2 -- the latter also the conv2 of ResidualBlockDown / Up
# --, ResidualBlockUp.conv1 and its shortcut), with the keywords the blocks pass
STRIDE1 = (Layer("bottleneck_in", 192, 96, 1, dict(ring=2)),
           Layer("bottleneck_3x3", 96, 96, 3, dict(pad=2, sphere=True, ring=2)),
           Layer("bottleneck_out", 96, 192, 1, dict(ring=2)),
           Layer("v2_conv1", 192, 192, 3, dict(pad=2, sphere=1, ring=1, ring_w=2)),
           Layer("v2_conv2", 192, 192, 3, dict(pad=2, sphere=2, ring=2)),
           Layer("up_conv1", 192, 768, 3, dict(pad=2, sphere=1, ring=2, crop=1, shuffle=True)),
           Layer("up_shortcut", 192, 768, 1, dict(ring=2, crop=1, shuffle=True)))
GATE = Layer("gate", 192, 192, 1, dict(ring=2))
STRIDE2 = (Layer("down_conv1", 192, 192, 3, {}), Layer("down_shortcut", 192, 192, 1, {}))
S2_KW = dict(pad=2, oring=2)                                               # what _sconv_s2 passes on


class Map(object):
    is_cuda, dtype, requires_grad = True, torch.float32, False

    def __init__(self, *shape):
        self.shape = shape

    def is_contiguous(self):
        return True


class Conv(object):
    def __init__(self, layer):
        self.weight, self.kernel_size, self.bias = torch.empty((layer.cout, layer.cin, layer.ks, layer.ks), device="meta"), (layer.ks, layer.ks), object()


def load_models(path):
    """lic360_models as the file at `path` has it, under a name of its own"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "360-image-compression_amd"))
    spec = importlib.util.spec_from_file_location("lic360_models_tabulated", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def routes(M):
    """{row: tokens} of the models module M"""
    lic360 = M.lic360
    public = [n for n in dir(lic360) if n.startswith("sconv") and not n.endswith(("_supported", "_pack")) and callable(getattr(lic360, n))]
    saved, calls = {n: getattr(lic360, n) for n in public}, []

    def recorder(name):
        def record(x, packed, bias, a, residual, out, **kw):
            calls.append((name, (x, packed, bias, a, residual, out), kw))
            return out
        return record

    saved_packed, M._packed = M._packed, lambda conv, precision, pack: (conv, precision, pack)
    for n in public:
        setattr(lic360, n, recorder(n))
    table = {}
    try:
        with torch.no_grad():
            def token(block, layer, n, hw, ask, call, kw):
                conv, x, a, res, out = Conv(layer), Map(n, layer.cin, *hw), object(), object(), object()
                answer = "." if ask is None else "ny"[bool(ask(conv, x))]
                del calls[:]
                assert call(block, conv, x, a, res, out, **kw) is out
                (name, args, got), = calls                                  # exactly one launch
                packed = args[1]
                assert args == (x, packed, conv.bias, a, res, out) and packed[0] is conv, (layer.name, name)
                assert packed[2] == "sconv%dx%d%s_pack" % (layer.ks, layer.ks, "" if packed[1] == "fp32" else "_" + packed[1]), (layer.name, packed[1:])
                narrow = {k: got.pop(k) for k in ("form", "cpw") if k in got}
                assert got == (kw or S2_KW) and (not narrow or len(narrow) == 2), (layer.name, name, got, narrow)    # the keywords travel unchanged
                return answer + name[len("sconv"):] + "".join(":%s" % narrow[k] for k in ("form", "cpw") if narrow) + "@" + packed[1]

            def row(key, block, layer, hw, ask, call, kw):
                assert key not in table, key
                table[key] = " ".join(token(block, layer, n, hw, ask, call, kw) for n in BATCHES)

            def ask1(layer, block):                                         # the block's question about a 3x3 stride-1 layer, as the blocks put it
                if layer.ks != 3:
                    return None
                return lambda conv, x: M._fusable(conv, x, layer.kw["ring"], layer.kw.get("ring_w"), mod=block)

            for precision in M.CONV_PRECISIONS:
                for small in M.SMALL_MODES:
                    block = M.set_conv_precision(torch.nn.Module(), precision, small=small)
                    for hw in MAPS:
                        mode = "%dx%d %s %s" % (hw + (precision, small))
                        for layer in STRIDE1:
                            row("%s %d>%d %s" % (layer.name, layer.cin, layer.cout, mode), block, layer, hw, ask1(layer, block), M._sconv, layer.kw)
                        row("gate 192>192 " + mode, block, GATE, hw, None, M._sconv_gate, GATE.kw)
            for stride2 in M.STRIDE2_PRECISIONS:                            # (the stride-1 precision is not theirs: bf16x3 throughout)
                block = M.set_conv_precision(torch.nn.Module(), "bf16x3", stride2=stride2)
                for hw in MAPS:
                    for layer in STRIDE2:
                        row("%s 192>192 %dx%d stride2=%s" % ((layer.name,) + hw + (stride2,)), block, layer, hw, lambda conv, x: M._fusable_s2(conv, x, block),
                            M._sconv_s2, {})
            # outside the supported shapes: 48 channels; the 96-channel 1x1 (no narrow gate at cout = 96); odd interiors
            block = M.set_conv_precision(torch.nn.Module(), "bf16x1", stride2="bf16x1", small="narrow")
            small3 = Layer("outside_48", 48, 48, 3, dict(pad=2, sphere=True, ring=2))
            row("outside_48 48>48 132x260 bf16x1 narrow", block, small3, (132, 260), ask1(small3, block), M._sconv, small3.kw)
            one96 = Layer("outside_96", 96, 96, 1, dict(ring=2))
            row("outside_96 96>96 132x260 bf16x1 narrow", block, one96, (132, 260), None, M._sconv, one96.kw)
            row("outside_96_gate 96>96 132x260 bf16x1 narrow", block, one96, (132, 260), None, M._sconv_gate, one96.kw)
            row("odd v2_conv2 192>192 133x261 bf16x1 narrow", block, STRIDE1[4], (133, 261), ask1(STRIDE1[4], block), M._sconv, STRIDE1[4].kw)
            for layer in STRIDE2:
                row("odd %s 192>192 259x515 stride2=bf16x1" % layer.name, block, layer, (259, 515), lambda conv, x: M._fusable_s2(conv, x, block),
                    M._sconv_s2, {})
            # a block set_conv_precision never touched
            bare = torch.nn.Module()
            row("bare v2_conv2 192>192 132x260", bare, STRIDE1[4], (132, 260), ask1(STRIDE1[4], bare), M._sconv, STRIDE1[4].kw)
            row("bare gate 192>192 132x260", bare, GATE, (132, 260), None, M._sconv_gate, GATE.kw)
            row("bare down_conv1 192>192 260x516", bare, STRIDE2[0], (260, 516), lambda conv, x: M._fusable_s2(conv, x, bare), M._sconv_s2, {})
    finally:
        M._packed = saved_packed
        for n, fn in saved.items():
            setattr(lic360, n, fn)
    return table


if __name__ == "__main__":
    json.dump(routes(load_models(sys.argv[1])), sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
