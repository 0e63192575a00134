"""The C ABI of the split-bf16 one-pass GDN (csrc/gdn_bf16x3.inc): the four entry points are exported by the library, declared in include/lic360_hip.h and
typed in lic360/_abi_table.py; the channel predicate; the argument contract refuses a bad call before any launch (no GPU is needed for a refusal: ARG_CHECK
returns first); and the transforms' setter carries the GDN precision per module, as a keyword that defaults to fp32."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lic360_gdn_bf16x3_supported", "lic360_gdn_bf16x3_packed_bytes", "lic360_gdn_bf16x3_pack", "lic360_gdn_bf16x3")


def test_the_four_symbols_are_exported():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                                 # dlsym on the library itself, not through the binding table
    for name in NAMES:
        assert getattr(raw, name) is not None, name
    for name in ("gdn_bf16x3_supported", "gdn_bf16x3_pack", "gdn_bf16x3_forward"):
        assert callable(getattr(lic360, name)), name


def test_they_are_in_the_header_and_in_the_table():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|long)\s+%s\s*\(" % name, header), name
        assert name in ABI, name
    i, p, l = "c_int", "c_void_p", "c_long"
    assert ABI["lic360_gdn_bf16x3_supported"] == (i, [i]) and ABI["lic360_gdn_bf16x3_packed_bytes"] == (l, [i])
    assert ABI["lic360_gdn_bf16x3_pack"] == (i, [p, p, p, i])
    assert ABI["lic360_gdn_bf16x3"] == ABI["lic360_gdn"] == (i, [p, p, p, p, p, i, i, l, i])      # stream, x, packed | gamma, beta, out; n, c, p, inverse


def test_the_channel_predicate():
    import lic360
    L = lic360._lib
    want = {16: 0, 32: 1, 48: 0, 64: 1, 96: 1, 100: 0, 128: 1, 192: 1, 224: 0}
    for c, ok in want.items():
        assert L.lic360_gdn_bf16x3_supported(c) == ok and lic360.gdn_bf16x3_supported(c) == bool(ok), c
        assert L.lic360_gdn_bf16x3_packed_bytes(c) == (4 * c * c if ok else 0), c
    assert all(lic360.gdn_supported(c) for c, ok in want.items() if ok)     # whatever the new form takes, the fp32 kernel takes too


def test_the_argument_contract_refuses_before_any_launch():
    """null operands, n <= 0, n > 65535, p <= 0, an unsupported c, a pack off a 16-byte boundary: each returns an error code and starts nothing (the
    pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16                                                          # a 16-byte aligned dummy address
    ok = dict(x=a, packed=a, beta=a, out=a, n=1, c=192, p=100, inverse=0)

    def call(**kw):
        v = dict(ok, **kw)
        return L.lic360_gdn_bf16x3(None, v["x"], v["packed"], v["beta"], v["out"], v["n"], v["c"], v["p"], v["inverse"])

    for k in ("x", "packed", "beta", "out"):
        assert call(**{k: None}) != 0, k
    assert call(n=0) != 0 and call(n=-1) != 0 and call(n=65536) != 0 and call(p=0) != 0 and call(p=-5) != 0
    for c in (0, 16, 48, 100, 224, -32):
        assert call(c=c) != 0, c
    assert call(packed=a + 4) != 0 and call(packed=a + 8) != 0
    assert b"bad argument" in L.lic360_last_error()
    assert L.lic360_gdn_bf16x3_pack(None, None, a, 192) != 0 and L.lic360_gdn_bf16x3_pack(None, a, None, 192) != 0
    assert L.lic360_gdn_bf16x3_pack(None, a, a, 48) != 0 and L.lic360_gdn_bf16x3_pack(None, a, a + 8, 192) != 0


def test_the_setter_carries_the_gdn_precision():
    import lic360_models as M
    assert M.GDN_PRECISIONS == ("fp32", "bf16x3")
    net = M.ResidualBlockDown(96, 96, 0)
    gdns = [m for m in net.modules() if type(m).__name__ == "GDN"]
    assert len(gdns) == 1 and not hasattr(gdns[0], "_gdn_precision")       # nothing set: GDN.forward reads "fp32"
    assert M.set_conv_precision(net, "fp32") is net
    mods = list(net.modules())
    assert len(mods) > 5 and all(m._gdn_precision == "fp32" for m in mods)  # the default
    M.set_conv_precision(net, "bf16x1", stride2="bf16x1", gdn="bf16x3")
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision) == ("bf16x1", "bf16x1", "bf16x3") for m in mods)
    M.set_conv_precision(net, "fp32", gdn="bf16x3")                         # independent of `precision` and `stride2`
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision) == ("fp32", "fp32", "bf16x3") for m in mods)
    for bad in ("bf16x1", "bf16", "FP32", None, 3):
        with pytest.raises(ValueError):
            M.set_conv_precision(net, "bf16x1", stride2="bf16x1", gdn=bad)
    with pytest.raises(ValueError):
        M.set_conv_precision(net, "bf16", gdn="bf16x3")
    with pytest.raises(ValueError):
        M.set_conv_precision(net, "bf16x1", stride2="bf16x3", gdn="bf16x3")
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision) == ("fp32", "fp32", "bf16x3") for m in mods)   # a refused call changes nothing
    M.set_conv_precision(net, "bf16x3", stride2="bf16x1")                   # without the keyword: back to fp32
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision) == ("bf16x3", "bf16x1", "fp32") for m in mods)
