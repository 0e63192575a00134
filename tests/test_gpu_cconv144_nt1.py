"""k_cconv144's one-tile decode-order instantiation (csrc/cconv144_kernels.hip: anti-diagonals whose window fits 16 rows) against the oracle,
bit for bit, next to the two-tile one: every class of window on one 20 x 15 map at batches where workgroups persist, and two chained layers whose
planes are launched in decode order, one-tile and two-tile launches mixed.  The cases and the rule that picks the kernel are in
tests/cconv144_nt1_cases.py; tests/test_cconv144_nt1_cases_cpu.py asserts that they reach what is claimed here.  Calling convention, layouts and
the case object as in tests/test_gpu_cconv144_batch.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cconv144_cases as cc
import cconv144_nt1_cases as n1
import oracle as orc
from test_gpu_cconv144_batch import _dc_call
from util import case_rng
from gpu_support import dev, host, lic  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", n1.DC_CASES, ids=n1.nt1_id)
def test_cconv144_dc_one_tile_planes_bit_exact(lic, case):
    """planes 0, 15, 16, 19 and 33 of a 20 x 15 map (one-tile: a one-row window, the largest that fits, th0 > 0, the last plane; two-tile: the
    smallest that does not fit), residual and PReLU on, into a buffer that starts as a finite sentinel: the launched anti-diagonals equal
    oracle + residual and every other float is still the sentinel.  The last layer also as the codec calls it: without a residual."""
    call = _dc_call(lic, case)
    try:
        for residual in (True,) if case[4] else (True, False):
            out = torch.full(call.shape, cc.SENTINEL, dtype=torch.float32, device="cuda:0")
            call.launch(out, residual)
            got, want = host(out), call.want(cc.SENTINEL, residual)
            assert (want != cc.SENTINEL).sum() > 0 and (want == cc.SENTINEL).mean() > 0.5
            assert np.array_equal(got, want), "residual %s: %s" % (residual, call.describe(got, want))
    finally:
        call.destroy()


def test_cconv144_dc_chained_layers_mix_one_and_two_tile_planes(lic):
    """x -> y -> z, two hidden layers with residual and PReLU on 33 maps of 20 x 15: for s = 14 .. 19 in decode order, on one stream, plane s of
    the first layer into y and then plane s of the second layer, which reads y's anti-diagonals s - 4 .. s as the launches so far left them
    (planes 14, 15, 18, 19 run the one-tile kernel, 16 and 17 the two-tile one), into z.  y (from zeros) and z (from the sentinel) equal the
    oracle's over the whole buffers."""
    N, H, W, planes = n1.CHAIN_N, n1.H, n1.W, n1.CHAIN_PLANES
    rng = case_rng(("nt1_chain", N, H, W) + planes)
    layers = [cc.i144_setup(lic, rng, 144, True) for _ in range(2)]
    x = rng.standard_normal((N, 144, H, W)).astype(np.float32)
    res = [rng.standard_normal((N, 144, H, W)).astype(np.float32) for _ in range(2)]
    L, P = lic._lib, lic._p
    rows, pitch = C.c_int(), C.c_int()
    assert L.lic360_dc144_layout(H, W, C.byref(rows), C.byref(pitch)) == 0
    rows, pitch = rows.value, pitch.value
    th, tw = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    on = np.isin(th + tw, planes)

    def skew(t, fill=0.0):
        o = np.full(t.shape[:2] + (rows, pitch), fill, np.float32)
        o[:, :, th + tw + cc.R0, th + cc.C0] = t
        return o
    # the oracle, in the same order: a plane of the second layer sees the planes of y computed so far (later ones are still zero)
    idx, pidx = orc.code_contex(H, W)
    y = np.zeros((N, 144, H, W), np.float32)
    z = np.zeros((N, 144, H, W), np.float32)
    for s in planes:
        cell = th + tw == s
        for src, dst, (w, b, a, plan, packed), r in ((x, y, layers[0], res[0]), (y, z, layers[1], res[1])):
            tmp = np.zeros_like(dst)
            orc.cconv_dc_plane(src, w, b, a, tmp, 1, 6, idx, pidx, s)
            dst[:, :, cell] = tmp[:, :, cell] + r[:, :, cell]
    assert not y[:, :, ~on].any() and not z[:, :, ~on].any()
    want_y = skew(y)
    want_z = np.full((N, 144, rows, pitch), cc.SENTINEL, np.float32)
    want_z[:, :, (th + tw + cc.R0)[on], (th + cc.C0)[on]] = z[:, :, on]
    xd, yd = dev(skew(x)), torch.zeros((N, 144, rows, pitch), dtype=torch.float32, device="cuda:0")
    zd = torch.full((N, 144, rows, pitch), cc.SENTINEL, dtype=torch.float32, device="cuda:0")
    rd = [dev(skew(r)) for r in res]
    keep = [(dev(b), dev(a)) for w, b, a, plan, packed in layers]
    try:
        for s in planes:
            for src, dst, (w, b, a, plan, packed), (bd, ad), r in ((xd, yd, layers[0], keep[0], rd[0]), (yd, zd, layers[1], keep[1], rd[1])):
                assert L.lic360_cconv144_dc_plane(lic._stream(0), plan, P(src), P(packed), P(bd), P(ad), P(r), P(dst), N, H, W, s) == 0, L.lic360_last_error()
        got_y, got_z = host(yd), host(zd)
    finally:
        torch.cuda.synchronize()
        for w, b, a, plan, packed in layers:
            L.lic360_conv_plan_destroy(plan)
    case = (N, H, W, 144, True, planes)
    assert np.array_equal(got_y, want_y), "first layer: " + cc.describe_dc_mismatch(case, got_y, want_y)
    assert np.array_equal(got_z, want_z), "second layer: " + cc.describe_dc_mismatch(case, got_z, want_z)
