"""The C entries of the fused viewport metrics' backward (include/lic360_hip.h, csrc/viewport_quality_kernels.hip) without a GPU: they are
exported with the argument contract of the binding table, every refusal comes before anything is launched, the plain entry's contract is what it
was, and the module takes its `grad` keyword."""
import ctypes

import pytest

COEF = ("c_int", ["c_void_p"] * 4 + ["c_int"] * 7 + ["c_void_p", "c_int"] + ["c_void_p"] * 7)
BACKWARD = ("c_int", ["c_void_p"] * 4 + ["c_int"] * 7 + ["c_void_p", "c_int"] + ["c_void_p"] * 10)
PLAIN = ("c_int", ["c_void_p"] * 4 + ["c_int"] * 7 + ["c_void_p", "c_int"] + ["c_void_p"] * 4)


def test_entries_are_exported_with_the_contract_of_the_table():
    import lic360
    from lic360._abi_table import ABI
    assert ABI["lic360_viewport_quality_coef"] == COEF and ABI["lic360_viewport_quality_backward"] == BACKWARD
    assert ABI["lic360_viewport_quality"] == PLAIN                  # the existing entry's tuple is unchanged
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                          # the built library itself, not the bound handle
    for name in ("lic360_viewport_quality_coef", "lic360_viewport_quality_backward"):
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI[name][1])
    assert callable(lic360.viewport_quality_coef) and callable(lic360.viewport_quality_backward)


def _host_buffers():
    """host addresses that are never read: every call below fails an ARG_CHECK.  One 1 MB block cut into slots of 64 KB, each larger than any
    buffer of the geometry used (n 1, c 1, ERP 8 x 16, views 5 x 7: at most 14 * 35 * 4 = 1960 bytes)"""
    block = (ctypes.c_double * (1 << 17))()
    base = (ctypes.addressof(block) + 15) // 16 * 16
    return block, lambda i: ctypes.c_void_p(base + i * 65536)


def test_coef_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    taps = (ctypes.c_float * 11)(*[1 / 11.0] * 11)
    good = dict(a=slot(0), b=slot(1), tf=slot(2), n=1, c=1, h=8, w=16, ho=5, wo=7, near=0, taps=taps, win=11, scratch=slot(3), mse=slot(4), ssim=slot(5),
                pa=slot(6), pb=slot(7), q=slot(8), r=slot(9))

    def call(**kw):
        g = dict(good, **kw)
        rc = L.lic360_viewport_quality_coef(None, g["a"], g["b"], g["tf"], g["n"], g["c"], g["h"], g["w"], g["ho"], g["wo"], g["near"], g["taps"], g["win"],
                                            g["scratch"], g["mse"], g["ssim"], g["pa"], g["pb"], g["q"], g["r"])
        return rc, L.lic360_last_error().decode()

    inside = lambda i, off: ctypes.c_void_p(slot(i).value + off)
    for kw in (dict(a=None), dict(b=None), dict(tf=None), dict(taps=None), dict(scratch=None), dict(mse=None), dict(ssim=None),   # the plain entry's checks
               dict(n=0), dict(c=0), dict(n=65536), dict(ho=0), dict(w=0), dict(win=10), dict(win=13), dict(win=0), dict(win=-1),
               dict(ssim=good["mse"]), dict(mse=good["scratch"]), dict(scratch=inside(3, 8)),
               dict(q=None), dict(r=None), dict(pa=None, pb=None),                                                               # the maps that are required
               dict(q=good["r"]), dict(pa=good["pb"]), dict(pa=inside(8, 4 * 34)), dict(pb=good["r"]),                           # maps overlap each other
               dict(q=good["mse"]), dict(r=good["ssim"]), dict(pa=good["scratch"]), dict(pb=inside(4, 4 * 13)),                  # a map over an output / the scratch
               dict(q=good["a"]), dict(pb=inside(1, 4 * 127))):                                                                  # a map over an input
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    del block


def test_backward_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    taps = (ctypes.c_float * 11)(*[1 / 11.0] * 11)
    good = dict(a=slot(0), b=slot(1), tf=slot(2), n=1, c=1, h=8, w=16, ho=5, wo=7, near=0, taps=taps, win=11, pa=slot(6), pb=slot(7), q=slot(8), r=slot(9),
                g_mse=slot(4), g_ssim=slot(5), ga=slot(10), gb=slot(11), va=slot(12), vb=slot(13))

    def call(**kw):
        g = dict(good, **kw)
        rc = L.lic360_viewport_quality_backward(None, g["a"], g["b"], g["tf"], g["n"], g["c"], g["h"], g["w"], g["ho"], g["wo"], g["near"], g["taps"], g["win"],
                                                g["pa"], g["pb"], g["q"], g["r"], g["g_mse"], g["g_ssim"], g["ga"], g["gb"], g["va"], g["vb"])
        return rc, L.lic360_last_error().decode()

    inside = lambda i, off: ctypes.c_void_p(slot(i).value + off)
    for kw in (dict(a=None), dict(b=None), dict(tf=None), dict(taps=None), dict(q=None), dict(r=None), dict(g_mse=None), dict(g_ssim=None),   # null pointers
               dict(n=0), dict(c=0), dict(n=65536), dict(ho=0), dict(w=0), dict(win=10), dict(win=13), dict(win=0), dict(win=-1),
               dict(ga=None, gb=None, pa=None, pb=None, va=None, vb=None),                                                       # no side at all
               dict(pa=None), dict(pb=None),                                                                                     # a gradient without its map ...
               dict(ga=None, va=None), dict(gb=None, vb=None),                                                                   # ... a map without its gradient
               dict(ga=None, pa=None), dict(gb=None, pb=None),                                                                   # the views of a side that is not live
               dict(ga=good["gb"]), dict(gb=inside(10, 4 * 127)), dict(va=good["vb"]), dict(va=good["ga"]),                      # outputs overlap each other
               dict(ga=good["a"]), dict(gb=inside(1, 4 * 127)), dict(ga=good["q"]), dict(gb=good["pa"]), dict(va=good["r"]),     # an output over an input
               dict(vb=good["pb"]), dict(ga=good["g_mse"]), dict(vb=inside(5, 4 * 13))):
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    del block


def test_module_takes_the_grad_keyword():
    """constructing needs no device; the default and the keyword left out are the library route, an unknown mode names the modes"""
    from lic360_operator import ViewportQuality
    assert ViewportQuality(16, 16, 0.4, False, 0).grad == "library" and ViewportQuality(16, 16, 0.4, False, 0, window_size=11, grad="library").grad == "library"
    assert ViewportQuality(16, 16, 0.4, False, 0, grad="fused").grad == "fused" and ViewportQuality.GRAD_MODES == ("library", "fused")
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        ViewportQuality(16, 16, 0.4, False, 0, grad="native")
