"""The C entries of the fused viewport metrics (include/lic360_hip.h, csrc/viewport_quality_kernels.hip) without a GPU: they are exported with the
argument contract of the binding table, the scratch query is the launch arithmetic, and the argument checks refuse before anything is launched."""
import ctypes

import pytest

import viewport_quality_cases as vq

ENTRY = ("c_int", ["c_void_p"] * 4 + ["c_int"] * 7 + ["c_void_p", "c_int"] + ["c_void_p"] * 4)
QUERY = ("c_long", ["c_int"] * 3)


def test_entries_are_exported_with_the_contract_of_the_table():
    import lic360
    from lic360._abi_table import ABI
    assert ABI["lic360_viewport_quality"] == ENTRY and ABI["lic360_viewport_quality_scratch_bytes"] == QUERY
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                         # the built library itself, not the bound handle
    for name in ("lic360_viewport_quality", "lic360_viewport_quality_scratch_bytes"):
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI[name][1])
    assert callable(lic360.viewport_quality) and callable(lic360.viewport_quality_scratch_bytes)
    import lic360_operator
    assert issubclass(lic360_operator.ViewportQuality, __import__("torch").nn.Module)


@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (3, 21, 37), (3, 5, 7), (8, 171, 256), (1, 17, 16)])
def test_scratch_query_is_the_launch_arithmetic(n, h, w):
    """one (ssim_sum, sq_sum) pair of doubles per 16 x 16 tile of each of the 14 viewports of each image"""
    import lic360
    tiles = -(-h // vq.TILE) * -(-w // vq.TILE)
    assert lic360.viewport_quality_scratch_bytes(n, h, w) == 16 * n * vq.NVIEW * tiles
    assert lic360._lib.lic360_viewport_quality_scratch_bytes(n, h, w) == 16 * n * vq.NVIEW * tiles


def test_scratch_query_refuses_with_zero():
    import lic360
    for args in ((0, 16, 16), (1, 0, 16), (1, 16, -1)):
        assert lic360.viewport_quality_scratch_bytes(*args) == 0


def test_argument_checks_refuse_before_any_launch():
    """every call below fails its ARG_CHECK, so nothing touches a device; the pointers are host addresses that are never read"""
    import lic360
    L = lic360._lib
    buf = (ctypes.c_double * 4096)()                                # 32 KB, 16-byte aligned or not: offsets below are multiples of 16
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    taps = (ctypes.c_float * 11)(*[1 / 11.0] * 11)
    a, b, tf, scratch, mse, ssim, smap = (ctypes.c_void_p(base + o) for o in (0, 16, 32, 1024, 64, 128, 8192))
    good = dict(a=a, b=b, tf=tf, n=1, c=1, h=8, w=16, ho=5, wo=7, near=0, taps=taps, win=11, scratch=scratch, mse=mse, ssim=ssim, smap=None)

    def call(**kw):
        g = dict(good, **kw)
        rc = L.lic360_viewport_quality(None, g["a"], g["b"], g["tf"], g["n"], g["c"], g["h"], g["w"], g["ho"], g["wo"], g["near"], g["taps"], g["win"],
                                       g["scratch"], g["mse"], g["ssim"], g["smap"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(a=None), dict(b=None), dict(tf=None), dict(taps=None), dict(scratch=None), dict(mse=None), dict(ssim=None),   # null pointers
               dict(n=0), dict(c=0), dict(n=65536), dict(ho=0), dict(w=0),                                                       # sizes
               dict(win=10), dict(win=13), dict(win=0), dict(win=-1),                                                            # window odd, at most 11
               dict(ssim=mse), dict(ssim=ctypes.c_void_p(base + 64 + 4 * 13)),                                                   # mse [1][14] and ssim overlap
               dict(mse=scratch), dict(ssim=ctypes.c_void_p(base + 1024 + 8)),                                                   # an output inside the scratch
               dict(smap=mse), dict(smap=ctypes.c_void_p(base + 1024 + 16)),                                                     # the map over an output / the scratch
               dict(scratch=ctypes.c_void_p(base + 1024 + 8))):                                                                  # misaligned scratch
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)


def test_table_query_tells_which_viewports_leave_the_erp():
    """lic360_projects_tf_inside is host arithmetic: a square viewport of fov 0.5 looks exactly at a pole with one row of the views pitched by 45
    degrees and leaves a 32 x 64 ERP there; the cases of the GPU test and the production geometry stay inside"""
    import lic360
    from lic360._abi_table import ABI
    from lic360_operator import MultiProject
    assert ABI["lic360_projects_tf_inside"] == ("c_int", ["c_int", "c_int", "c_void_p", "c_void_p", "c_float", "c_int", "c_int", "c_int"])
    th, ph = (ctypes.c_float * 14)(*MultiProject.THETAS), (ctypes.c_float * 14)(*MultiProject.PHIS)
    inside = lambda ho, wo, fov, h, w, near: lic360._lib.lic360_projects_tf_inside(ho, wo, th, ph, ctypes.c_float(fov), h, w, near)
    assert inside(16, 16, 0.5, 32, 64, 0) == 0
    for case in vq.CASES:
        assert inside(case.view[0], case.view[1], case.fov, case.erp[0], case.erp[1], int(case.near)) == 1, case.name
    assert inside(171, 256, 0.5, 512, 1024, 0) == 1 and inside(171, 256, 0.5, 512, 1024, 1) == 1
    assert inside(1, 16, 0.5, 32, 64, 0) == -1 and inside(16, 16, 0.5, 0, 64, 0) == -1 and lic360._lib.lic360_projects_tf_inside(16, 16, None, ph, ctypes.c_float(0.5), 32, 64, 0) == -1
    op = lic360.ProjectsOp(16, 16, list(MultiProject.THETAS), list(MultiProject.PHIS), 0.5, False, 0)
    assert op._table_inside(32, 64) is False and lic360.ProjectsOp(16, 16, list(MultiProject.THETAS), list(MultiProject.PHIS), 0.4, False, 0)._table_inside(32, 64) is True
