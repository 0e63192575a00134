"""The C entries of the group-causal convolution's weight gradient (include/lic360_hip_grad.h, csrc/cconv_wgrad_kernels.hip) without a GPU: declared in
the new header, present in the second binding table, bound and exported, the first table unchanged; the scratch query positive, monotone and 0 for
refused or empty arguments; every refusal before anything is launched; MaskConv2 and the three models take their keywords."""
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WGRAD = ("c_int", ["c_void_p"] * 5 + ["c_int"] * 8)
SCRATCH = ("c_long", ["c_int"] * 8)
NAMES = ("lic360_cconv_wgrad", "lic360_cconv_wgrad_scratch_bytes")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_abi", os.path.join(ROOT, "tools", "gen_abi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_entries_are_declared_bound_and_exported():
    import lic360
    from lic360._abi_table import ABI
    from lic360._abi_table_grad import ABI_GRAD
    header = open(os.path.join(ROOT, "include", "lic360_hip_grad.h")).read()
    first = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header) and not re.search(r"\b%s\b" % name, first), name
    assert ABI_GRAD == {"lic360_cconv_wgrad": WGRAD, "lic360_cconv_wgrad_scratch_bytes": SCRATCH}
    assert len(ABI) == 167 and not set(ABI) & set(ABI_GRAD)
    g = _gen()
    assert g.parse(open(g.HEADER).read()) == ABI and g.parse(open(g.HEADER_GRAD).read()) == ABI_GRAD, "run tools/gen_abi.py after editing a header"
    assert g.OUT.endswith("_abi_table.py") and g.OUT_GRAD.endswith("_abi_table_grad.py")
    assert open(g.OUT_GRAD).read() == g.render(ABI_GRAD, "lic360_hip_grad.h", "ABI_GRAD") and open(g.OUT).read() == g.render(ABI)
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                          # the built library itself, not the bound handle
    for name in NAMES:
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI_GRAD[name][1])
    with pytest.raises(ctypes.ArgumentError):                       # bound with the range check: not truncated
        lic360._lib.lic360_cconv_wgrad_scratch_bytes(2 ** 40, 4, 4, 4, 4, 1, 5, 6)
    for fn in ("cconv_wgrad", "cconv_dgrad", "cconv_forward", "cconv_wgrad_scratch_bytes", "cconv_group_flip", "cconv_transpose_weight"):
        assert callable(getattr(lic360, fn)), fn


def test_scratch_bytes_is_positive_and_monotone():
    import lic360
    q = lic360._lib.lic360_cconv_wgrad_scratch_bytes
    # one group of 4 -> 4 channels is one pair whose live taps are th + tw <= 4 (15 tiles; 10 under constrain 5), one split: 16 bytes of table + the tiles
    assert q(1, 4, 4, 1, 1, 1, 5, 6) == 16 + 15 * 1024 and q(1, 4, 4, 1, 1, 1, 5, 5) == 16 + 10 * 1024
    base = dict(n=2, channel=24, nout=18, h=9, w=35)
    for k in ("n", "h", "w"):
        prev = 0
        for v in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64, 65, 128, 129, 600, 5000):
            a = dict(base, **{k: v})
            cur = q(a["n"], a["channel"], a["nout"], a["h"], a["w"], 6, 5, 6)
            assert cur > 0 and cur >= prev, (a, cur, prev)
            prev = cur
        assert k == "w" or prev > q(base["n"], base["channel"], base["nout"], base["h"], base["w"], 6, 5, 6)      # n and h do grow it; w does not enter
    prev = 0
    for G in (1, 2, 3, 6, 12, 48, 96):                                          # more groups of the same 4 -> 3 form
        cur = q(2, 4 * G, 3 * G, 9, 35, G, 5, 6)
        assert cur > prev, (G, cur, prev)
        prev = cur
    good = (2, 24, 18, 9, 35, 6, 5, 6)
    assert q(*good) > 0
    for k, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, -1), (1, -24), (2, -18), (3, -9), (4, -35), (5, 0), (5, -6), (6, 3), (6, 7), (7, 4), (7, 7),
                 (5, 5), (5, 4), (0, 2 ** 31 - 1), (3, 2 ** 31 - 1)):
        a = list(good)
        a[k] = v
        assert q(*a) == 0, a                                                   # refused or empty
    assert q(65536, 24, 18, 65536, 35, 6, 5, 6) == 0 and q(1, 2 ** 20 * 16, 2 ** 20 * 16, 1, 1, 1, 5, 6) == 0


def _host_buffers():
    """host addresses that are never read: every call below is refused, or is a no-op"""
    block = (ctypes.c_double * (1 << 16))()
    base = (ctypes.addressof(block) + 15) // 16 * 16
    return block, lambda i: ctypes.c_void_p(base + i * 65536)


def test_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    good = dict(x=slot(0), gy=slot(1), gw=slot(2), scratch=slot(3), n=2, channel=24, nout=18, h=3, w=4, ngroup=6, ksz=5, constrain=6)

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_cconv_wgrad(None, a["x"], a["gy"], a["gw"], a["scratch"], a["n"], a["channel"], a["nout"], a["h"], a["w"], a["ngroup"], a["ksz"],
                                  a["constrain"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(x=None), dict(gy=None), dict(gw=None), dict(scratch=None),                                                       # null pointers
               dict(n=-1), dict(channel=-24), dict(nout=-18), dict(h=-3), dict(w=-4), dict(ngroup=0), dict(ngroup=-6),               # negative sizes
               dict(ksz=3), dict(ksz=7), dict(ksz=0), dict(n=0, ksz=3),                                                              # ksz != 5, also without an image
               dict(constrain=4), dict(constrain=7), dict(constrain=0), dict(n=0, constrain=4),                                      # constrain outside {5, 6}
               dict(ngroup=5), dict(channel=25), dict(nout=19), dict(n=0, nout=19),                                                  # not divisible by ngroup
               dict(n=65536, h=65536), dict(n=2 ** 31 - 1, h=2 ** 31 - 1), dict(h=2 ** 31 - 1, w=2 ** 31 - 1),                      # products that overflow
               dict(channel=2 ** 20 * 18, nout=2 ** 20 * 18), dict(n=2 ** 30, h=1, w=2 ** 30),
               dict(h=0, gw=None), dict(w=0, gw=None),                                                                               # an empty sum still writes gw
               dict(scratch=ctypes.c_void_p(slot(3).value + 8)), dict(scratch=ctypes.c_void_p(slot(3).value + 4))):                  # scratch off 16 bytes
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0), dict(n=0, x=None, gy=None, gw=None, scratch=None), dict(channel=0, x=None, gw=None), dict(nout=0, gy=None, gw=None)):
        rc, msg = call(**kw)                                                    # no image, or an empty gw: no error, nothing launched
        assert rc == 0, (kw, rc, msg)
    del block


def test_modules_take_their_keywords():
    """constructing needs no device; an unknown route names the routes; both routes hold the same state"""
    from lic360_operator import MaskConv2
    import lic360_models as lm
    assert MaskConv2.ROUTES == ("library", "fused")
    assert MaskConv2(6, 4, 3, 5, True).route == "library" and MaskConv2(6, 4, 3, 5, True, 0, False, "fused").route == "fused"
    assert MaskConv2(6, 1, 4, 5, route="fused").constrain == 5 and MaskConv2(6, 4, 4, 5, True, route="fused").constrain == 6
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        MaskConv2(6, 4, 3, 5, True, route="native")
    a, b = MaskConv2(6, 4, 3, 5, True), MaskConv2(6, 4, 3, 5, True, route="fused")
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"] and a.weight.shape == b.weight.shape == (18, 24, 5, 5)
    for make in (lambda **k: lm.EntropyResidualBlock(6, 4, **k), lambda **k: lm.EntropyNet2(6, 4, 3, **k), lambda **k: lm.EntropyNet3(1, 12, 6, **k)):
        lib, fused = make(), make(conv="fused")
        convs = lambda net: [m for m in net.modules() if isinstance(m, MaskConv2)]
        assert convs(lib) and all(m.route == "library" for m in convs(lib)) and all(m.route == "fused" for m in convs(fused))
        assert len(convs(lib)) == len(convs(fused))
        assert list(lib.state_dict()) == list(fused.state_dict())
        assert [tuple(v.shape) for v in lib.state_dict().values()] == [tuple(v.shape) for v in fused.state_dict().values()]
        with pytest.raises(ValueError, match="'library'.*'fused'"):
            make(conv="native")
    assert lm.EntropyNet2(6, 4, 3, head="fused", conv="fused").head.route == "fused" and lm.EntropyNet3(1, 12, 6, conv="fused").head.route == "library"
