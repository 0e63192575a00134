"""The fused viewport metrics (csrc/viewport_quality_kernels.hip, lic360.viewport_quality, lic360_operator.ViewportQuality) against the fp32
restatement of tests/viewport_quality_cases.py: both images are projected with ProjectsOp.forward (pinned by the oracle in tests/test_gpu_ops.py),
the restatement runs on those views on the CPU, and the fused call must give its per-cell SSIM map bit for bit and its per-viewport means
within one fp32 ulp (the double sums differ only in their order, far below an fp32 ulp).  Plus: sentinel-filled buffers, two streams,
identical inputs, the library fallback of the module, the refusal of a table that leaves the ERP."""
import numpy as np
import pytest
import torch

import viewport_quality_cases as vq
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _op(lic, case):
    from lic360_operator import MultiProject
    return lic.ProjectsOp(case.view[0], case.view[1], list(MultiProject.THETAS), list(MultiProject.PHIS), case.fov, case.near, 0)


def _assert_table_stays_inside(tf, h, w, near):
    """every index the sampling forms from the table lies inside one ERP plane (checked on the host before any kernel samples with it: where a
    viewport row looks exactly at a pole, e.g. a square viewport of fov 0.5, the longitude of the table leaves [0, w - 1])"""
    x, y = tf[..., 0].astype(np.float64), tf[..., 1].astype(np.float64)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    if near:
        tw, th = np.fmod(np.floor(x + 0.5), w), np.minimum(np.floor(y + 0.5), h - 1)
        lo, hi = th * w + tw, th * w + tw
    else:
        tw, th = np.floor(x), np.floor(y)
        pw, ph = np.fmod(tw + 1, w), np.minimum(th + 1, h - 1)
        lo, hi = th * w + np.minimum(tw, pw), ph * w + np.maximum(tw, pw)
    assert lo.min() >= 0 and hi.max() < h * w, (lo.min(), hi.max(), h * w)


@pytest.fixture(scope="module")
def results(lic):
    """per case, computed once and left unchanged: the device inputs, the projected views (CPU), the restatement, the fused outputs (CPU)"""
    out = {}
    for case in vq.CASES:
        a, b = (torch.from_numpy(x).cuda() for x in vq.make_erp_pair(case))
        op, taps = _op(lic, case), vq.taps_of(case.window)
        assert op._table_inside(*case.erp)                                               # the library's own host check, and an independent one
        _assert_table_stays_inside(op._coords(a, *case.erp).cpu().numpy(), case.erp[0], case.erp[1], case.near)
        va = op.forward(a)[0].cpu().numpy()
        vb = op.forward(b)[0].cpu().numpy()
        fused = tuple(t.cpu().numpy() for t in lic.viewport_quality(op, a, b, taps, return_map=True))
        out[case.name] = dict(a=a, b=b, op=op, taps=taps, va=va, vb=vb, ref=vq.ref_quality(va, vb, taps), fused=fused)
    torch.cuda.synchronize()
    return out


def _ulps(x, ref):
    return np.abs(x.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("case", vq.CASES, ids=[c.name for c in vq.CASES])
def test_fused_call_matches_the_restatement(results, case):
    r = results[case.name]
    (mse, ssim, m), (mse_ref, ssim_ref, m_ref) = r["fused"], r["ref"]
    assert m.shape == m_ref.shape == (vq.NVIEW * case.n, case.c) + case.view and mse.shape == ssim.shape == (case.n, vq.NVIEW)
    assert np.isfinite(m_ref).all() and np.ptp(ssim_ref) > 0                             # the viewports differ: a mixed-up order would show
    diff = m.view(np.uint32) != m_ref.view(np.uint32)
    print("%s: map cells that differ %d of %d; mse up to %.3g ulp, ssim up to %.3g ulp" % (
        case.name, int(diff.sum()), diff.size, _ulps(mse, mse_ref).max(), _ulps(ssim, ssim_ref).max()))
    assert not diff.any(), "first differing cell %s: %r vs %r" % (np.argwhere(diff)[0], m[diff][0], m_ref[diff][0])
    assert _ulps(mse, mse_ref).max() <= 1 and _ulps(ssim, ssim_ref).max() <= 1


def test_outputs_do_not_depend_on_what_the_buffers_held(lic, results):
    case = vq.CASES[1]
    r = results[case.name]
    n, (h, w) = case.n, case.view
    got = []
    for fill in (0x00, 0xFF):                                                            # zeros, and the all-ones pattern (a NaN in every float and double)
        buf = lambda *shape: torch.full(shape, fill, dtype=torch.uint8, device="cuda:0")
        mse, ssim, smap = (buf(*s, 4).view(torch.float32).squeeze(-1) for s in ((n, 14), (n, 14), (14 * n, case.c, h, w)))
        scratch = buf(lic.viewport_quality_scratch_bytes(n, h, w))
        res = lic.viewport_quality(r["op"], r["a"], r["b"], r["taps"], mse=mse, ssim=ssim, ssim_map=smap, scratch=scratch)
        assert res[0] is mse and res[1] is ssim and res[2] is smap
        got.append([t.cpu().numpy() for t in res])
    for x, y, z in zip(got[0], got[1], r["fused"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
    mse, ssim = (t.cpu().numpy() for t in lic.viewport_quality(r["op"], r["a"], r["b"], r["taps"]))         # without the map: the same means
    assert np.array_equal(mse, r["fused"][0]) and np.array_equal(ssim, r["fused"][1])


def test_two_streams_keep_their_own_results(lic, results):
    r1, r2 = results["partial_tiles"], results["production"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    got = []
    for _ in range(3):
        for s, r in zip(streams, (r1, r2)):
            with torch.cuda.stream(s):
                got.append((r, lic.viewport_quality(r["op"], r["a"], r["b"], r["taps"], return_map=True)))
    torch.cuda.synchronize()
    for r, res in got:
        for x, y in zip(res, r["fused"]):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("case", vq.CASES, ids=[c.name for c in vq.CASES])
def test_identical_inputs_give_exactly_one_and_zero(lic, results, case):
    r = results[case.name]
    mse, ssim, m = lic.viewport_quality(r["op"], r["a"], r["a"].clone(), r["taps"], return_map=True)
    assert bool((m == 1.0).all()) and bool((ssim == 1.0).all()) and bool((mse == 0.0).all())


def test_module_runs_the_fused_call_and_its_fallback_agrees(lic, results):
    """The module on device tensors is the fused call; on CPU tensors, on other dtypes and in a recording pass it takes MultiProject + SSIM +
    torch.mean (the library's convolution).  Bound: the float64 bound of tests/test_viewport_quality_cases_cpu.py, 4 times the yardstick y -- the
    deviation of the library's fp32 SSIM / fp32 mean on the CPU from a float64 evaluation -- measured here on this case's own views, per viewport,
    for each of the three fallback variants."""
    from lic360_operator import ViewportQuality
    case = vq.CASES[1]
    r = results[case.name]
    q = ViewportQuality(case.view[0], case.view[1], case.fov, case.near, 0, window_size=case.window)
    mse, ssim, m = q(r["a"], r["b"], return_map=True)
    for x, y in zip((mse, ssim, m), r["fused"]):
        assert x.is_cuda and np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))
    mse64, ssim64 = vq.f64_quality(r["va"], r["vb"], r["taps"])
    mse_lib, ssim_lib = vq.library_quality(r["va"], r["vb"], case.window)
    y_mse, y_ssim = float(np.abs(mse_lib - mse64).max()), float(np.abs(ssim_lib - ssim64).max())
    assert y_mse > 0 and y_ssim > 0
    fb_mse, fb_ssim, fb_map = q(r["a"].cpu(), r["b"].cpu(), return_map=True)
    assert not fb_mse.is_cuda and not fb_map.is_cuda and fb_mse.shape == fb_ssim.shape == (case.n, 14) and fb_map.shape == m.shape
    g_mse, g_ssim = q(r["a"].clone().requires_grad_(), r["b"])
    assert g_ssim.requires_grad and g_mse.requires_grad
    h_mse, h_ssim = q(r["a"].double(), r["b"].double())
    assert h_ssim.is_cuda and not h_ssim.requires_grad and not h_mse.requires_grad
    for name, v_mse, v_ssim in (("cpu tensors", fb_mse, fb_ssim), ("recording pass", g_mse, g_ssim), ("float64 tensors", h_mse, h_ssim)):
        d_mse = float(np.abs(v_mse.detach().cpu().numpy().astype(np.float64) - r["fused"][0]).max())
        d_ssim = float(np.abs(v_ssim.detach().cpu().numpy().astype(np.float64) - r["fused"][1]).max())
        print("%s vs fused, per viewport: mse %.3e (yardstick %.3e), ssim %.3e (yardstick %.3e)" % (name, d_mse, y_mse, d_ssim, y_ssim))
        assert d_mse <= 4 * y_mse and d_ssim <= 4 * y_ssim, name


def test_a_table_that_leaves_the_erp_is_refused(lic, results):
    """a square viewport of fov 0.5 has, in the views pitched by 45 degrees, a row that looks exactly at a pole: its table indexes outside the ERP
    plane, and the fused call refuses it on the host instead of sampling with it (the refusal comes before anything is uploaded or launched)"""
    from lic360_operator import MultiProject, ViewportQuality
    r = results["one_tile"]
    op = lic.ProjectsOp(16, 16, list(MultiProject.THETAS), list(MultiProject.PHIS), 0.5, False, 0)
    assert not op._table_inside(32, 64) and r["op"]._table_inside(32, 64)
    with pytest.raises(lic.Lic360Error, match="sample outside"):
        lic.viewport_quality(op, r["a"], r["b"], r["taps"])
    with pytest.raises(lic.Lic360Error, match="sample outside"):
        ViewportQuality(16, 16, 0.5, False, 0)(r["a"], r["b"])
    assert op._tf is None                                                                 # nothing was uploaded for it
