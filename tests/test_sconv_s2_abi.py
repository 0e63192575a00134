"""The C ABI of the stride-2 sphere convolutions (csrc/conv3x3_kernels.hip): the four entry points are exported by the library, declared in
include/lic360_hip.h and typed in lic360/_abi_table.py; their shape predicates are the stride-1 ones; the argument contract refuses a bad call
before any launch (no GPU is needed for a refusal: ARG_CHECK returns first)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lic360_sconv3x3s2_supported", "lic360_sconv3x3s2", "lic360_sconv1x1s2_supported", "lic360_sconv1x1s2")


def test_the_four_symbols_are_exported():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                                 # dlsym on the library itself, not through the binding table
    for name in NAMES:
        assert getattr(raw, name) is not None, name


def test_they_are_in_the_header_and_in_the_table():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in ABI, name
    i, p = "c_int", "c_void_p"
    assert ABI["lic360_sconv3x3s2_supported"] == (i, [i, i]) and ABI["lic360_sconv1x1s2_supported"] == (i, [i, i])
    assert ABI["lic360_sconv3x3s2"] == (i, [p] * 7 + [i] * 8)              # stream, x, packed, bias, slope, residual, out; n, cin, cout, hp, wp, pad, sphere, oring
    assert ABI["lic360_sconv1x1s2"] == (i, [p] * 7 + [i] * 7)              # ...; n, cin, cout, hp, wp, pad, oring


def test_shape_predicates_are_the_stride_1_ones():
    import lic360
    L = lic360._lib
    assert L.lic360_sconv3x3s2_supported(192, 192) == 1 and L.lic360_sconv3x3s2_supported(96, 96) == 1
    assert L.lic360_sconv3x3s2_supported(3, 192) == 0 and L.lic360_sconv3x3s2_supported(192, 100) == 0
    assert L.lic360_sconv1x1s2_supported(16, 192) == 0 and L.lic360_sconv1x1s2_supported(32, 192) == 1
    for cin in (3, 16, 32, 48, 96, 192, 200):
        for cout in (48, 96, 100, 192, 384, 768):
            assert L.lic360_sconv3x3s2_supported(cin, cout) == L.lic360_sconv3x3_supported(cin, cout)
            assert L.lic360_sconv1x1s2_supported(cin, cout) == L.lic360_sconv1x1_supported(cin, cout)
    assert lic360.sconv3x3s2_supported(192, 192) and not lic360.sconv1x1s2_supported(16, 192)


def test_the_argument_contract_refuses_before_any_launch():
    """odd interiors, a sphere rule without an apron, a chunk past 32-bit byte offsets, misaligned bias / slope, null operands: each returns an
    error code and starts nothing (the pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16                                                          # a 16-byte aligned dummy address
    ok3 = dict(n=1, cin=32, cout=192, hp=36, wp=36, pad=2, sphere=1, oring=2)

    def call3(bias=a, slope=None, x=a, **kw):
        v = dict(ok3, **kw)
        return L.lic360_sconv3x3s2(None, x, a, bias, slope, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["pad"], v["sphere"], v["oring"])

    def call1(bias=a, **kw):
        v = dict(ok3, **kw)
        return L.lic360_sconv1x1s2(None, a, a, bias, None, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["pad"], v["oring"])

    assert call3(hp=37) != 0 and call3(wp=35) != 0 and call1(hp=37) != 0 and call1(wp=35) != 0        # odd interiors
    assert call3(pad=0, hp=32, wp=32) != 0 and call3(pad=0, sphere=0, hp=32, wp=32) != 0             # the 3x3 reaches one apron row / column
    assert call3(hp=4 + 2 * 16384, wp=4 + 2 * 16384) != 0 and call1(hp=4 + 2 * 16384, wp=4 + 2 * 16384) != 0     # a chunk's plane set >= 2^32 bytes
    assert call3(bias=a + 4) != 0 and call3(slope=a + 8) != 0 and call1(bias=a + 4) != 0               # 16-byte operand loads
    assert call3(x=None) != 0 and call3(n=0) != 0 and call3(cin=3) != 0 and call3(cout=100) != 0 and call1(cin=16) != 0
    assert call3(sphere=2) != 0 and call3(oring=-1) != 0
