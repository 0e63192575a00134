"""The first decode layer with its three nets in one task per image (k_cconv4v6<1, false, false, 3> / k_cconv4v6t<1, 3>, csrc/cconv4v6_dc.inc)
against the CPU oracle, bit for bit, through lic360_cconv4_dc_plane, plane by plane, on the cases of tests/dc_first_nets_cases.py
(tests/test_dc_first_nets_cpu.py shows which launch each case reaches).  The three nets read ONE input of B images (x_mod = B); the output of
3 B samples starts from a sentinel, so a cell that is written off-plane, at another net's samples, or not at all shows up.

Mutations that must fail here (scratch builds, reported with the change that added the kernels): every net computing with net 0's weights; every
net storing at net 0's sample index."""
import ctypes as C

import numpy as np
import pytest
import torch

import dc_first_nets_cases as cases
import oracle as orc
import ref_codec as rc
from util import conv_params, latent
from gpu_support import dev, lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _first_layer_planes(lic, G, H, W, N, nb, x_mod, planes, residual, checks):
    """one first layer (cin = 1, cout = 4, PReLU, constraint 5) of nb nets over N samples that read x_mod inputs, on the planes given; the persistent
    output is compared with the oracle's after every plane of `checks` and after the last one"""
    cout, constrain = 4, 5
    rng = np.random.default_rng(5000 + 7 * G + 131 * N + 17 * H + W + nb)
    nout = G * cout
    w, b, a = conv_params(rng, nb if nb > 1 else None, nout, G, act=True)
    if nb == 1:
        w, b, a = w[None], b[None], a[None]
    x = rng.standard_normal((x_mod, G, H, W)).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = 0.0
    res = rng.standard_normal((N, nout, H, W)).astype(np.float32) if residual else None
    L = lic._lib
    rows, pitch, row0, col0 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert L.lic360_dc4_layout(H, W, C.byref(rows), C.byref(pitch), C.byref(row0), C.byref(col0)) == 0
    rows, pitch, row0, col0 = rows.value, pitch.value, row0.value, col0.value
    th, tw = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def skew(t, fill=0.0):
        o = np.full(t.shape[:2] + (rows, pitch), fill, np.float32)
        o[:, :, th + tw + row0, th + col0] = t
        return o

    def to_dev(t):                                                         # planes + the slack the band fetches may touch
        buf = torch.zeros(L.lic360_conv4_buffer_floats(0, t.shape[0] * t.shape[1], H, W), dtype=torch.float32, device="cuda:0")
        buf[:t.size] = torch.from_numpy(t.reshape(-1)).to("cuda:0")
        return buf
    plan = C.c_void_p(0)
    assert L.lic360_conv_plan_create(G, G, nout, 5, constrain, C.byref(plan)) == 0
    assert L.lic360_conv4_supported(plan) == 1
    packed = torch.empty(nb * L.lic360_conv4_packed_floats(plan), dtype=torch.float32, device="cuda:0")
    wd, bd, ad = dev(w), dev(b), dev(a)
    xd = to_dev(skew(x))
    rd = to_dev(skew(res)) if residual else None
    out = torch.full((L.lic360_conv4_buffer_floats(0, N * nout, H, W),), cases.SENTINEL, dtype=torch.float32, device="cuda:0")
    s, P = lic._stream(0), lic._p
    assert L.lic360_conv4_pack(s, plan, P(wd), nb, P(packed)) == 0, L.lic360_last_error()
    idx, pidx = orc.code_contex(H, W)
    xo = np.ascontiguousarray(np.tile(x, (N // x_mod, 1, 1, 1)))          # the oracle's sample i reads x[i]
    ref = np.zeros((N, nout, H, W), np.float32)
    done = np.zeros((1, nout, H, W), bool)
    g = np.arange(G).repeat(cout)[None, :, None, None]
    for p in planes:
        orc.cconv_dc_plane(xo, w, b, a, ref, G, constrain, idx, pidx, p)
        done |= (th + tw)[None, None] + g == p
        assert L.lic360_cconv4_dc_plane(s, plan, P(xd), P(packed), P(bd), P(ad), P(rd), P(out), N, H, W, nb, p, x_mod) == 0, L.lic360_last_error()
        if p in checks or p == planes[-1]:
            got = out.cpu().numpy()[:N * nout * rows * pitch].reshape(N, nout, rows, pitch)
            want = skew(np.where(done, ref + res if residual else ref, cases.SENTINEL).astype(np.float32), cases.SENTINEL)
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                n_, o_, r_, c_ = (int(v) for v in bad[0])
                raise AssertionError("plane %d: %d cells differ; first: sample %d (net %d, image %d), channel %d, cell (%d, %d): got %r, want %r" % (
                    p, len(bad), n_, n_ // (N // nb), n_ % (N // nb), o_, c_ - col0, r_ - row0 - (c_ - col0), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))
    L.lic360_conv_plan_destroy(plan)


@pytest.mark.parametrize("case", cases.MERGED_CASES, ids=cases.case_id)
def test_first_layer_three_nets_per_task_bit_exact(lic, case):
    """tapes of 2, 3 and 6 images (64-row windows cut at 61 rows), plain tasks over uneven XCD lists, the full-length planes of the bench's latent
    shape, and the one-double-step tasks of G = 6 back to back in a workgroup (plain: 324 images; taped: 320 and 640), each run once"""
    G, H, W, B, planes, residual = case
    planes = cases.planes_of(case)
    checks = {G} if case[4] is None and B < 100 else set()              # (and after the last plane)
    _first_layer_planes(lic, G, H, W, 3 * B, 3, B, planes, residual, checks)


@pytest.mark.parametrize("case", cases.OLD_FORM_CASES, ids=lambda c: "g%d_%dx%d_n%d_nb%d_xmod%d" % c)
def test_other_first_layer_launches_keep_the_one_net_kernels(lic, case):
    """three nets with an input each (x_mod = n) and a single net: the one-net kernels, the oracle's result"""
    G, H, W, N, nb, x_mod = case
    _first_layer_planes(lic, G, H, W, N, nb, x_mod, tuple(range(H + W + G - 2)), True, {G})


@pytest.mark.parametrize("G,H,W,B", cases.CODEC_CASES, ids=lambda v: str(v))
def test_fused_codec_round_trip_with_merged_first_layer(lic, G, H, W, B):
    """FusedCodec at batches whose first decode layer runs merged (tapes of 2 and of 3 images): the oracle's bytes, the oracle's symbols"""
    from lic360_fused import FusedCodec
    rng = np.random.default_rng(900 + B)
    layers = rc.make_main_params(2900 + B, G)
    items = [latent(rng, G, H, W) for _ in range(B)]
    code = np.concatenate([it[0] for it in items], 0)
    mask = np.concatenate([it[1] for it in items], 0)
    ref = [rc.encode_main(code[i:i + 1], mask[i:i + 1], layers, G) for i in range(B)]
    fc = FusedCodec(G, H, W, max_batch=B)
    fc.load_layers(layers)
    streams = fc.encode(dev(code), dev(mask))
    assert streams == ref
    out = fc.decode(streams, dev(mask)).cpu().numpy()
    assert np.array_equal(out, code * mask)
    assert np.array_equal(rc.decode_main(ref[0], mask[0:1], layers, G), (code * mask)[0:1])
