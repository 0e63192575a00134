"""The C ABI of the attention blocks' fused gate (csrc/conv3x3_kernels.hip, k_gate_sconv*): the three entry points are exported by the library, declared in
include/lic360_hip.h and typed in lic360/_abi_table.py with 14 arguments each; the argument contract refuses a bad call before any launch (no GPU is needed
for a refusal: ARG_CHECK returns first); and the transforms' setter carries the gate mode per module, as a keyword that defaults to "library"."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lic360_sconv1x1_gate", "lic360_sconv1x1_gate_bf16x3", "lic360_sconv1x1_gate_bf16x1")


def test_the_three_symbols_are_exported():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                                 # dlsym on the library itself, not through the binding table
    for name in NAMES:
        assert getattr(raw, name) is not None, name
        assert callable(getattr(lic360, name[len("lic360_"):])), name


def test_they_are_in_the_header_and_in_the_table():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    i, p = "c_int", "c_void_p"
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert ABI[name] == (i, [p] * 7 + [i] * 7), name                    # stream, x, packed, bias, trunk, residual, out; n, cin, cout, hp, wp, ring, ring_w
        assert len(ABI[name][1]) == 14
    assert "test/model_zoo.py:25-46" in header[header.index("k_gate_sconv"):header.index("int lic360_sconv1x1_gate(")]


def test_the_argument_contract_refuses_before_any_launch():
    """an unsupported shape, a null trunk, a null residual, a bf16 pack off a 16-byte boundary, and the 1x1 launch's other refusals: each returns an error code
    and starts nothing (the pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16                                                          # a 16-byte aligned dummy address
    ok = dict(x=a, packed=a, bias=a, trunk=a, residual=a, out=a, n=1, cin=192, cout=192, hp=20, wp=36, ring=2, ring_w=2)

    for name in NAMES:
        def call(**kw):
            v = dict(ok, **kw)
            return getattr(L, name)(None, v["x"], v["packed"], v["bias"], v["trunk"], v["residual"], v["out"], v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["ring"],
                                    v["ring_w"])
        for k in ("x", "packed", "bias", "trunk", "residual", "out"):
            assert call(**{k: None}) != 0, (name, k)
            assert b"bad argument" in L.lic360_last_error()
        for cin, cout in ((48, 192), (16, 192), (192, 48), (192, 288), (0, 192), (192, 0)):
            assert call(cin=cin, cout=cout) != 0, (name, cin, cout)
        assert call(n=0) != 0 and call(hp=4) != 0 and call(wp=4) != 0 and call(ring=-1) != 0 and call(ring=3, ring_w=2) != 0
        assert call(bias=a + 4) != 0 and call(bias=a + 8) != 0
        assert call(hp=1 << 14, wp=1 << 14) != 0                            # a chunk's cells past 32-bit byte offsets
        if name != NAMES[0]:
            assert call(packed=a + 4) != 0 and call(packed=a + 8) != 0


def test_the_setter_carries_the_gate_mode():
    import lic360_models as M
    assert M.GATE_MODES == ("library", "fused")
    net = M.AttentionBlock(96, 0)
    assert not hasattr(net, "_gate_mode")                                   # nothing set: forward reads "library"
    assert M.set_conv_precision(net, "fp32") is net
    mods = list(net.modules())
    assert len(mods) > 5 and all(m._gate_mode == "library" for m in mods)   # the default
    assert M.set_conv_precision(net, "bf16x1", stride2="bf16x1", gdn="bf16x3", gate="fused") is net
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision, m._gate_mode) == ("bf16x1", "bf16x1", "bf16x3", "fused") for m in mods)
    M.set_conv_precision(net, "fp32", gate="fused")                         # independent of the other keywords
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision, m._gate_mode) == ("fp32", "fp32", "fp32", "fused") for m in mods)
    for bad in ("fp32", "Fused", "on", None, 1, True):
        with pytest.raises(ValueError):
            M.set_conv_precision(net, "bf16x1", gate=bad)
    with pytest.raises(ValueError):
        M.set_conv_precision(net, "bf16", gate="fused")
    assert all((m._conv_precision, m._gate_mode) == ("fp32", "fused") for m in mods)       # a refused call changes nothing
    M.set_conv_precision(net, "bf16x3", gdn="bf16x3")                       # without the keyword: back to the library
    assert all((m._conv_precision, m._gdn_precision, m._gate_mode) == ("bf16x3", "bf16x3", "library") for m in mods)
