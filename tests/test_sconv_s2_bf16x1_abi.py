"""The C ABI of the single-pass bf16 forms of the stride-2 sphere convolutions (csrc/conv3x3_kernels.hip, csrc/sconv_b1s2.inc): the four entry points are
exported by the library, declared in include/lic360_hip.h and typed in lic360/_abi_table.py with the fp32 stride-2 argument lists; their shape predicates
are the stride-1 bf16x1 ones; the argument contract refuses a bad call before any launch (no GPU is needed for a refusal: ARG_CHECK returns first); and
the transforms' setter carries the stride-2 precision per module, as a keyword that defaults to fp32."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lic360_sconv3x3s2_bf16x1_supported", "lic360_sconv3x3s2_bf16x1", "lic360_sconv1x1s2_bf16x1_supported", "lic360_sconv1x1s2_bf16x1")


def test_the_four_symbols_are_exported():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                                 # dlsym on the library itself, not through the binding table
    for name in NAMES:
        assert getattr(raw, name) is not None, name
    for name in ("sconv3x3s2_bf16x1_supported", "sconv3x3s2_bf16x1", "sconv1x1s2_bf16x1_supported", "sconv1x1s2_bf16x1"):
        assert callable(getattr(lic360, name)), name


def test_they_are_in_the_header_and_in_the_table():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in ABI, name
    i = "c_int"
    assert ABI["lic360_sconv3x3s2_bf16x1_supported"] == (i, [i, i]) and ABI["lic360_sconv1x1s2_bf16x1_supported"] == (i, [i, i])
    assert ABI["lic360_sconv3x3s2_bf16x1"] == ABI["lic360_sconv3x3s2"]     # stream, x, packed, bias, slope, residual, out; n, cin, cout, hp, wp, pad, sphere, oring
    assert ABI["lic360_sconv1x1s2_bf16x1"] == ABI["lic360_sconv1x1s2"]     # ...; n, cin, cout, hp, wp, pad, oring
    assert len(ABI["lic360_sconv3x3s2_bf16x1"][1]) == 15 and len(ABI["lic360_sconv1x1s2_bf16x1"][1]) == 14


def test_shape_predicates_are_the_stride_1_bf16x1_ones():
    import lic360
    L = lic360._lib
    assert L.lic360_sconv3x3s2_bf16x1_supported(192, 192) == 1 and L.lic360_sconv3x3s2_bf16x1_supported(96, 96) == 1
    assert L.lic360_sconv3x3s2_bf16x1_supported(16, 192) == 0 and L.lic360_sconv1x1s2_bf16x1_supported(32, 192) == 1
    for cin in (3, 16, 32, 48, 96, 192, 200):
        for cout in (48, 96, 100, 192, 384, 768):
            assert L.lic360_sconv3x3s2_bf16x1_supported(cin, cout) == L.lic360_sconv3x3_bf16x1_supported(cin, cout)
            assert L.lic360_sconv1x1s2_bf16x1_supported(cin, cout) == L.lic360_sconv1x1_bf16x1_supported(cin, cout)
    assert lic360.sconv3x3s2_bf16x1_supported(192, 192) and not lic360.sconv3x3s2_bf16x1_supported(16, 192) and not lic360.sconv1x1s2_bf16x1_supported(16, 192)


def test_the_argument_contract_refuses_before_any_launch():
    """the refusals of tests/test_sconv_s2_abi.py -- odd interiors, a 3x3 without an apron, a chunk past 32-bit byte offsets (now 32 channels), misaligned
    bias / slope, null operands, bad shapes and flags -- plus 16 input channels for the 3x3 and a misaligned pack: each returns an error code and starts
    nothing (the pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16                                                          # a 16-byte aligned dummy address
    ok3 = dict(n=1, cin=32, cout=192, hp=36, wp=36, pad=2, sphere=1, oring=2)

    def call3(bias=a, slope=None, x=a, packed=a, **kw):
        v = dict(ok3, **kw)
        return L.lic360_sconv3x3s2_bf16x1(None, x, packed, bias, slope, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["pad"], v["sphere"], v["oring"])

    def call1(bias=a, packed=a, **kw):
        v = dict(ok3, **kw)
        return L.lic360_sconv1x1s2_bf16x1(None, a, packed, bias, None, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["pad"], v["oring"])

    assert call3(hp=37) != 0 and call3(wp=35) != 0 and call1(hp=37) != 0 and call1(wp=35) != 0        # odd interiors
    assert call3(pad=0, hp=32, wp=32) != 0 and call3(pad=0, sphere=0, hp=32, wp=32) != 0             # the 3x3 reaches one apron row / column
    assert call3(hp=4 + 2 * 16384, wp=4 + 2 * 16384) != 0 and call1(hp=4 + 2 * 16384, wp=4 + 2 * 16384) != 0     # a chunk's plane set >= 2^32 bytes
    assert call3(hp=4 + 2 * 2896, wp=4 + 2 * 2896) != 0                     # 32 x 5796^2 x 4 bytes: past 2^32 with the 32-channel chunk (16 channels would fit)
    assert call3(bias=a + 4) != 0 and call3(slope=a + 8) != 0 and call1(bias=a + 4) != 0               # 16-byte operand loads
    assert call3(packed=a + 8) != 0 and call1(packed=a + 4) != 0 and call3(packed=None) != 0          # the pack is read in 16-byte cells
    assert call3(x=None) != 0 and call3(n=0) != 0 and call3(cin=3) != 0 and call3(cout=100) != 0 and call1(cin=16) != 0
    assert call3(cin=16) != 0 and call3(cin=48) != 0                        # the 3x3's chunk is 32 channels in this form
    assert call3(sphere=2) != 0 and call3(oring=-1) != 0


def test_the_setter_carries_the_stride_2_precision():
    import lic360_models as M
    assert M.CONV_PRECISIONS == ("fp32", "bf16x3", "bf16x1") and M.STRIDE2_PRECISIONS == ("fp32", "bf16x1")
    net = M.ResidualBlockDown(96, 96, 0)
    assert M.set_conv_precision(net, "bf16x1", stride2="bf16x1") is net
    mods = list(net.modules())
    assert len(mods) > 5 and all(m._stride2_precision == "bf16x1" and m._conv_precision == "bf16x1" for m in mods)
    M.set_conv_precision(net, "fp32", stride2="bf16x1")                     # independent of the stride-1 precision
    assert all(m._stride2_precision == "bf16x1" and m._conv_precision == "fp32" for m in mods)
    for bad in ("bf16x3", "bf16", None, 1):
        with pytest.raises(ValueError):
            M.set_conv_precision(net, "fp32", stride2=bad)
    assert all(m._stride2_precision == "bf16x1" for m in mods)             # a refused call changes nothing
    with pytest.raises(ValueError):
        M.set_conv_precision(net, "bf16", stride2="bf16x1")
    M.set_conv_precision(net, "bf16x1")                                     # without the keyword: back to fp32
    assert all(m._stride2_precision == "fp32" and m._conv_precision == "bf16x1" for m in mods)
