"""The C ABI of the single-pass bf16 ("bf16x1") sphere convolutions (csrc/conv3x3_kernels.hip, csrc/sconv_bf16x3.inc): the eight entry points are
exported by the library, declared in include/lic360_hip.h and typed in lic360/_abi_table.py with the argument lists of their bf16x3 counterparts; the
shape predicate is bf16x3's; a pack is cout cin ks^2 2 bytes; the models know the mode.  No GPU: nothing is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple("lic360_sconv%s_bf16x1%s" % (k, s) for k in ("3x3", "1x1") for s in ("_supported", "_packed_bytes", "_pack", ""))


def test_the_eight_symbols_are_exported():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                                 # dlsym on the library itself, not through the binding table
    assert len(NAMES) == 8
    for name in NAMES:
        assert getattr(raw, name) is not None, name


def test_they_are_in_the_header_and_typed_as_their_bf16x3_counterparts():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|long)\s+%s\s*\(" % name, header), name
        assert name in ABI, name
        assert ABI[name] == ABI[name.replace("bf16x1", "bf16x3")], name
    i, p = "c_int", "c_void_p"
    assert ABI["lic360_sconv3x3_bf16x1"] == (i, [p] * 7 + [i] * 11)        # stream, x, packed, bias, slope, residual, out; n, cin, cout, hp, wp, pad, sphere, ring, ring_w, crop, shuffle
    assert ABI["lic360_sconv1x1_bf16x1"] == (i, [p] * 7 + [i] * 9)
    assert ABI["lic360_sconv3x3_bf16x1_packed_bytes"] == ("c_long", [i, i]) and ABI["lic360_sconv1x1_bf16x1_pack"] == (i, [p, p, p, i, i])


def test_shape_predicate_and_pack_size():
    import lic360
    L = lic360._lib
    for cin in (3, 16, 32, 48, 64, 96, 192, 200, 384):
        for cout in (48, 96, 100, 192, 288, 384, 768):
            for ks, k in ((3, "3x3"), (1, "1x1")):
                ok = getattr(L, "lic360_sconv%s_bf16x3_supported" % k)(cin, cout)
                assert ok == (1 if cin % 32 == 0 and (cout == 96 or cout % 192 == 0) else 0), (cin, cout)
                assert getattr(L, "lic360_sconv%s_bf16x1_supported" % k)(cin, cout) == ok, (k, cin, cout)
                assert getattr(L, "lic360_sconv%s_bf16x1_packed_bytes" % k)(cin, cout) == (cout * cin * ks * ks * 2 if ok else 0), (k, cin, cout)
                assert getattr(lic360, "sconv%s_bf16x1_supported" % k)(cin, cout) is bool(ok)
    assert L.lic360_sconv3x3_bf16x1_packed_bytes(192, 192) * 2 == L.lic360_sconv3x3_bf16x3_packed_bytes(192, 192)


def test_the_argument_contract_refuses_before_any_launch():
    """unsupported channels, a ring below the taps' reach, a misaligned pack or bias, null operands: each returns an error code and starts nothing
    (the pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = dict(n=1, cin=32, cout=192, hp=36, wp=36, pad=2, sphere=1, ring=2, ring_w=2, crop=0, shuffle=0)

    def call3(x=a, packed=a, bias=a, **kw):
        v = dict(ok, **kw)
        return L.lic360_sconv3x3_bf16x1(None, x, packed, bias, None, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["pad"], v["sphere"], v["ring"],
                                        v["ring_w"], v["crop"], v["shuffle"])

    def call1(packed=a, **kw):
        v = dict(ok, **kw)
        return L.lic360_sconv1x1_bf16x1(None, a, packed, a, None, None, a, v["n"], v["cin"], v["cout"], v["hp"], v["wp"], v["ring"], v["ring_w"], v["crop"], v["shuffle"])

    assert call3(cin=16) != 0 and call3(cout=100) != 0 and call1(cin=48) != 0 and call3(n=0) != 0 and call3(x=None) != 0
    assert call3(ring=0) != 0 and call3(crop=3) != 0 and call3(ring_w=1) != 0 and call3(sphere=3) != 0
    assert call3(packed=a + 4) != 0 and call1(packed=a + 8) != 0 and call3(bias=a + 4) != 0          # 16-byte operand loads
    assert L.lic360_sconv3x3_bf16x1_pack(None, a, a + 4, 32, 192) != 0 and L.lic360_sconv1x1_bf16x1_pack(None, a, a, 16, 192) != 0


def test_the_models_know_the_mode():
    import lic360_models as lm
    assert lm.CONV_PRECISIONS == ("fp32", "bf16x3", "bf16x1")
    for ks in (3, 1):
        fn, pack, ok = lm._SCONV[ks, "bf16x1"]
        assert (fn, pack, ok) == ("sconv%dx%d_bf16x1" % (ks, ks), "sconv%dx%d_bf16x1_pack" % (ks, ks), "sconv%dx%d_bf16x1_supported" % (ks, ks))
    m = lm.ResidualBlockV2(192, 0)
    assert lm.set_conv_precision(m, "bf16x1") is m and all(s._conv_precision == "bf16x1" for s in m.modules())
    for bad in ("bf16", "BF16X1", None):
        with pytest.raises(ValueError):
            lm.set_conv_precision(m, bad)
