"""The C ABI of the narrow-workgroup sphere convolutions (csrc/conv3x3_kernels.hip, k_narrow_conv / k_narrow_gate): three entry points serve every form,
kernel size and width -- exported by the library, declared in include/lic360_hip.h, typed in lic360/_abi_table.py; the argument contract refuses a bad call
before any launch (no GPU is needed for a refusal: ARG_CHECK returns first): an unknown form, cpw outside {48, 96}, cpw not below the pack's block, and what the
wide launches refuse; and the transforms' setter carries the small-launch mode per module, as a keyword that defaults to "library"."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lic360_sconv_narrow_supported", "lic360_sconv_narrow", "lic360_sconv1x1_gate_narrow")


def test_the_symbols_are_exported_and_wrapped():
    import lic360
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None, name
    for fn in ("sconv3x3_narrow", "sconv1x1_narrow", "sconv1x1_gate_narrow", "sconv_narrow_supported"):
        assert callable(getattr(lic360, fn)), fn


def test_they_are_in_the_header_and_in_the_table():
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    i, p = "c_int", "c_void_p"
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert ABI[NAMES[0]] == (i, [i] * 5)                                    # form, ks, cin, cout, cpw
    assert ABI[NAMES[1]] == (i, [p] + [i] * 3 + [p] * 6 + [i] * 11)         # stream; form, ks, cpw; x .. out; n, cin, cout, hp, wp, pad, sphere, ring, ring_w, out_crop, shuffle
    assert ABI[NAMES[2]] == (i, [p] + [i] * 2 + [p] * 6 + [i] * 7)          # stream; form, cpw; x, packed, bias, trunk, residual, out; n, cin, cout, hp, wp, ring, ring_w
    assert len([n for n in ABI if "narrow" in n]) == 3                      # a small set of entry points, not one per form x size


def test_the_predicate():
    import lic360
    S = lic360.sconv_narrow_supported
    for form in ("fp32", "bf16x3", "bf16x1"):
        for ks in (3, 1):
            assert S(form, ks, 192, 192, 96) and S(form, ks, 192, 192, 48) and S(form, ks, 96, 96, 48) and S(form, ks, 192, 768, 48)
            assert not S(form, ks, 96, 96, 96) and not S(form, ks, 192, 192, 192) and not S(form, ks, 192, 192, 24) and not S(form, ks, 192, 192, 144)
            assert not S(form, ks, 192, 288, 48) and not S(form, ks, 8, 192, 48) and not S(form, 5, 192, 192, 48)
    assert S("fp32", 3, 16, 96, 48) and not S("bf16x3", 3, 16, 96, 48) and not S("bf16x1", 3, 16, 96, 48)      # the forms' own chunks
    assert not S("fp16", 3, 192, 192, 96)
    assert not lic360._lib.lic360_sconv_narrow_supported(2, 3, 192, 192, 96) and lic360._lib.lic360_sconv_narrow_supported(3, 3, 192, 192, 96)


def test_the_argument_contract_refuses_before_any_launch():
    """each refusal returns an error code and starts nothing (the pointers are never dereferenced on the host; no device is touched)"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = dict(form=0, ks=3, cpw=96, x=a, packed=a, bias=a, slope=a, residual=None, trunk=a, out=a, n=1, cin=192, cout=192, hp=20, wp=36, pad=2, sphere=1, ring=2, ring_w=2,
              crop=0, shuffle=0)

    def conv(**kw):
        v = dict(ok, **kw)
        return L.lic360_sconv_narrow(None, v["form"], v["ks"], v["cpw"], v["x"], v["packed"], v["bias"], v["slope"], v["residual"], v["out"], v["n"], v["cin"], v["cout"],
                                     v["hp"], v["wp"], v["pad"], v["sphere"], v["ring"], v["ring_w"], v["crop"], v["shuffle"])

    def gate(**kw):
        v = dict(dict(ok, residual=a), **kw)
        return L.lic360_sconv1x1_gate_narrow(None, v["form"], v["cpw"], v["x"], v["packed"], v["bias"], v["trunk"], v["residual"], v["out"], v["n"], v["cin"], v["cout"],
                                             v["hp"], v["wp"], v["ring"], v["ring_w"])

    for call in (conv, gate):
        for form in (0, 3, 1):
            for bad in (dict(form=2), dict(form=-1), dict(form=4), dict(cpw=0), dict(cpw=24), dict(cpw=144), dict(cpw=192), dict(cpw=384)):
                assert call(**dict(dict(form=form), **bad)) != 0, (call.__name__, form, bad)
                assert b"bad argument" in L.lic360_last_error()
            for k in ("x", "packed", "bias", "out"):
                assert call(form=form, **{k: None}) != 0, (call.__name__, k)
            for cin, cout in ((48, 192), (16, 192), (192, 48), (192, 288), (0, 192), (192, 0)):
                assert call(form=form, cin=cin, cout=cout) != 0, (call.__name__, cin, cout)
            assert call(form=form, n=0) != 0 and call(form=form, hp=4) != 0 and call(form=form, wp=4) != 0 and call(form=form, ring=-1) != 0
            assert call(form=form, ring=3, ring_w=2) != 0 and call(form=form, bias=a + 4) != 0
            assert call(form=form, hp=1 << 14, wp=1 << 14) != 0             # a chunk's cells past 32-bit byte offsets
            if form:
                assert call(form=form, packed=a + 8) != 0                   # a bf16 pack off a 16-byte boundary
    assert conv(cout=96, cin=96, cpw=96) != 0 and gate(cout=96, cin=96, cpw=48) != 0       # not below the 96-block; the gate takes cout % 192 == 0
    assert gate(trunk=None) != 0 and gate(residual=None) != 0
    assert conv(ks=5) != 0 and conv(ks=1, pad=2, sphere=1) != 0
    assert conv(sphere=3) != 0 and conv(pad=0) != 0 and conv(crop=3) != 0 and conv(residual=a, crop=1) != 0 and conv(shuffle=1, out=a + 4) != 0 and conv(slope=a + 4) != 0


def test_the_setter_carries_the_small_launch_mode():
    import lic360_models as M
    assert M.SMALL_MODES == ("library", "narrow") and M.NARROW_CPWS == (96, 48)
    net = M.AttentionBlock(96, 0)
    assert not hasattr(net, "_small_mode")                                  # nothing set: forward reads "library"
    assert M.set_conv_precision(net, "fp32") is net
    mods = list(net.modules())
    assert len(mods) > 5 and all(m._small_mode == "library" for m in mods)  # the default
    assert M.set_conv_precision(net, "bf16x1", stride2="bf16x1", gdn="bf16x3", gate="fused", small="narrow") is net
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision, m._gate_mode, m._small_mode) == ("bf16x1", "bf16x1", "bf16x3", "fused", "narrow") for m in mods)
    M.set_conv_precision(net, "fp32", small="narrow")                       # independent of the other keywords
    assert all((m._conv_precision, m._stride2_precision, m._gdn_precision, m._gate_mode, m._small_mode) == ("fp32", "fp32", "fp32", "library", "narrow") for m in mods)
    for bad in ("fp32", "Narrow", "on", None, 1, True):
        with pytest.raises(ValueError) as e:
            M.set_conv_precision(net, "bf16x1", small=bad)
        assert "small-launch mode must be one of ('library', 'narrow')" in str(e.value)
    with pytest.raises(ValueError):
        M.set_conv_precision(net, "bf16", small="narrow")
    assert all((m._conv_precision, m._small_mode) == ("fp32", "narrow") for m in mods)     # a refused call changes nothing
    M.set_conv_precision(net, "bf16x3", gate="fused")                       # without the keyword: back to the library
    assert all((m._conv_precision, m._gate_mode, m._small_mode) == ("bf16x3", "fused", "library") for m in mods)


def test_the_count_rule_picks_the_widest_width_that_fills_the_chip():
    """_narrow_cpw on the production shapes (no GPU: shape arithmetic and the library's predicates): a 132 x 260 map at batch 1, a map the wide kernel takes"""
    import lic360_models as M
    blk = M.set_conv_precision(M.ResidualBlockV2(192, 0), "fp32", small="narrow")
    lib = M.set_conv_precision(M.ResidualBlockV2(192, 0), "fp32")
    assert M._narrow_cpw(blk, 3, 192, 192, 1, 128, 256) == 96               # 128 tiles x 2 = 256 workgroups
    assert M._narrow_cpw(blk, 3, 96, 96, 1, 128, 256) == 48
    # routed back by measurement: the fp32 3x3 at cpw 96 with a tall last tile row (ResidualBlockV2.conv1's 130-row window) -- and not retried at cpw 48
    assert M.NARROW_ROUTED_BACK == {("fp32", 3, 96, True)} and M.NARROW_MIN_WORKGROUPS == 256
    assert M._narrow_cpw(blk, 3, 192, 192, 1, 130, 256) is None
    for p in ("bf16x3", "bf16x1"):
        assert M._narrow_cpw(M.set_conv_precision(M.ResidualBlockV2(192, 0), p, small="narrow"), 3, 192, 192, 1, 130, 256) == 96
    assert M._narrow_cpw(blk, 3, 192, 192, 8, 34, 64) == 48                 # 36 x 68 at batch 8: tall at cpw 48, taken in fp32
    assert M._narrow_cpw(M.set_conv_precision(M.ResidualBlockV2(192, 0), "bf16x3", small="narrow"), 3, 192, 192, 8, 34, 64) is None     # no tall row: 384, 75 % of two rounds
    assert M._narrow_cpw(blk, 3, 96, 96, 8, 32, 64) is None                 # 128 workgroups: below the floor
    assert M._narrow_cpw(blk, 1, 192, 96, 1, 128, 256) == 48 and M._narrow_cpw(blk, 1, 96, 192, 1, 128, 256) == 96
    assert M._narrow_cpw(blk, 3, 192, 192, 1, 256, 512) is None             # the wide kernel takes it: no narrow call
    assert M._narrow_cpw(blk, 3, 192, 768, 1, 128, 256) is None             # 128 x 4 wide workgroups
    assert M._narrow_cpw(lib, 3, 192, 192, 1, 128, 256) is None and M._narrow_cpw(M.ResidualBlockV2(192, 0), 3, 192, 192, 1, 128, 256) is None
    assert M._narrow_cpw(blk, 3, 192, 192, 1, 8, 8) is None                 # no width fills the chip
    assert M._narrow_cpw(blk, 3, 48, 48, 1, 128, 256) is None               # a shape the kernels do not take
