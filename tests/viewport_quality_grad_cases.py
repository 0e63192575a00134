"""Cases and an fp32 restatement of the backward of the fused viewport metrics (csrc/viewport_quality_kernels.hip: k_viewport_quality<.., COEF>,
k_viewport_quality_backward; lic360.viewport_quality_coef / viewport_quality_backward).  No GPU in here: tests/test_viewport_quality_grad_cases_cpu.py
checks this file by itself, tests/test_gpu_viewport_quality_grad.py compares the kernels with it.  The cases are those of
tests/viewport_quality_cases.py and one of their size with asymmetric normalised taps, the only thing that notices an unreversed window.

All of the following in numpy fp32, one rounding per operation, on two stacks of projected views [14 n, c, h, w] (viewport-major):
  * ref_coefs: the window sums mu_a, mu_b, E_aa, E_bb, E_ab and the SSIM m of the forward's restatement, then
        A1 = 2 mu_a mu_b + c1    A2 = 2 (E_ab - mu_a mu_b) + c2    B1 = mu_a^2 + mu_b^2 + c1    B2 = var_a + var_b + c2    den = B1 B2    m = (A1 A2) / den
        t1 = m / B1    t2 = m / B2    u = (A2 - A1) / den    dt = t2 - t1
        Q = -t2    R = (2 A1) / den    Pa = 2 (mu_b u + mu_a dt)    Pb = 2 (mu_a u + mu_b dt)
  * ref_view_grads: blurT of a map = the forward's row pass then column pass with the taps in reversed index order (ascending over the reversed
    taps, from a zero accumulator, one rounded product and one rounded sum each) over the map padded with win // 2 zeros a side; then, with
    gs = g_ssim[img, v] / (float)N and gm = g_mse[img, v] / (float)N, N = c h w, in this order:
        t = bPa + (2 * xa) * bQ;    t = t + xb * bR;    gva = gs * t + gm * (2 * (xa - xb))
        t = bPb + (2 * xb) * bQ;    t = t + xa * bR;    gvb = gs * t + gm * (2 * (xb - xa))
    Its keyword arguments switch in the five kernel mistakes tests/test_viewport_quality_grad_cases_cpu.py shows it is sensitive to.
  * scatter_sums: the products weight * weight * gv of lic360_project_scatter in fp32 from a downloaded table, and per ERP cell their float64 sum, the
    sum of their magnitudes and their number: fp32 summation of n terms in any order lies within n * 2^-24 * sum |terms| of the exact sum (first order).

Deviation from float64 (torch_view_grads in float64: autograd over f64_quality's formula), measured by tests/test_viewport_quality_grad_cases_cpu.py over
all the cases below, largest absolute difference of a view gradient over the largest float64 gradient of the case:
    restatement 4.0e-06, torch's fp32 autograd of the same formula on the CPU (library convolution) 1.07e-05
(both on the production case, b = a + noise, where SSIM's denominators are smallest; the other cases 1.7e-07 ... 8.9e-07 against 3.0e-07 ... 1.5e-06.
The yardstick is the second number; the restatement is allowed 4x that, case by case)."""
import numpy as np

import viewport_quality_cases as vq

NVIEW = vq.NVIEW
CASES = list(vq.CASES) + [vq.Case("asymmetric_taps", (32, 64), (21, 37), 1, 3, False, 11, "uniform", 7)]


def taps_of(case):
    """the case's fp32 1-D window: the Gaussian of lic360_operator.extras, or, for the asymmetric case, random positive taps normalised in fp32"""
    if case.name != "asymmetric_taps":
        return vq.taps_of(case.window)
    t = np.random.default_rng(case.seed).random(case.window, dtype=np.float32) + np.float32(0.05)
    t = t / t.sum(dtype=np.float32)
    assert t.dtype == np.float32 and not np.array_equal(t, t[::-1])
    return t


def upstream(case):
    """(g_mse, g_ssim) [n, 14] fp32: random per (image, viewport), of both signs, with one exact zero each"""
    rng = np.random.default_rng(1000 + case.seed)
    g_mse, g_ssim = (rng.standard_normal((case.n, NVIEW)).astype(np.float32) for _ in range(2))
    g_mse[0, 5], g_ssim[0, 3] = 0.0, 0.0
    assert (g_mse < 0).any() and (g_ssim < 0).any()
    return g_mse, g_ssim


def _shape(va, vb, taps):
    va, vb, taps = np.ascontiguousarray(va, np.float32), np.ascontiguousarray(vb, np.float32), np.asarray(taps, np.float32)
    assert va.shape == vb.shape and va.ndim == 4 and va.shape[0] % NVIEW == 0 and len(taps) % 2 == 1
    return va, vb, taps, va.shape[0] // NVIEW, va.shape[1:], len(taps) // 2


def ref_coefs(va, vb, taps):
    """(Pa, Pb, Q, R), each [14 n, c, h, w] fp32, in the operation order of the module docstring"""
    va, vb, taps, n, (c, h, w), r = _shape(va, vb, taps)
    pad = ((0, 0), (0, 0), (r, r), (r, r))
    pa, pb = np.pad(va, pad), np.pad(vb, pad)
    two, c1, c2 = np.float32(2), np.float32(0.01 ** 2), np.float32(0.03 ** 2)
    blur = lambda p: vq._window_pass(p, taps, h, w)
    mu_a, mu_b, e_aa, e_bb, e_ab = blur(pa), blur(pb), blur(pa * pa), blur(pb * pb), blur(pa * pb)
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    a1, a2, b1, b2 = two * mu_a * mu_b + c1, two * cov + c2, mu_a * mu_a + mu_b * mu_b + c1, var_a + var_b + c2
    den = b1 * b2
    m = (a1 * a2) / den
    t1, t2, u = m / b1, m / b2, (a2 - a1) / den
    dt = t2 - t1
    out = two * (mu_b * u + mu_a * dt), two * (mu_a * u + mu_b * dt), -t2, (two * a1) / den
    assert all(x.dtype == np.float32 for x in out)
    return out


def _blur_t(x, taps, r, reverse, halo, padding):
    h, w = x.shape[-2:]
    pad = ((0, 0), (0, 0), (r, r), (r, r))
    p = np.pad(x, pad, mode="reflect") if padding == "reflect" and r else np.pad(x, pad)
    t = taps[::-1] if reverse else taps
    if halo is None:
        return vq._window_pass(p, t, h, w)
    out, cut = np.zeros(x.shape, np.float32), max(r - halo, 0)          # tile by tile: what lies more than `halo` cells outside the tile reads 0
    for y0 in range(0, h, vq.TILE):
        for x0 in range(0, w, vq.TILE):
            th, tw = min(vq.TILE, h - y0), min(vq.TILE, w - x0)
            q = p[..., y0:y0 + th + 2 * r, x0:x0 + tw + 2 * r].copy()
            if cut:
                q[..., :cut, :] = 0
                q[..., -cut:, :] = 0
                q[..., :, :cut] = 0
                q[..., :, -cut:] = 0
            out[..., y0:y0 + th, x0:x0 + tw] = vq._window_pass(q, t, th, tw)
    return out


def ref_view_grads(va, vb, taps, coefs, g_mse, g_ssim, reverse=True, halo=None, padding="zero", padded_count=False, q_factor=2):
    """(gva, gvb), each [14 n, c, h, w] fp32, from the maps `coefs` = (Pa, Pb, Q, R) and the upstream gradients [n, 14].  The keyword arguments are
    kernel mistakes: reverse=False applies the forward's window instead of its adjoint; halo=k loads only k cells of the maps around each 16 x 16 tile;
    padding="reflect" mirrors the maps at the viewport's border instead of reading 0; padded_count divides by the cells of the whole tiles;
    q_factor=1 drops the factor 2 of the E_aa / E_bb term."""
    va, vb, taps, n, (c, h, w), r = _shape(va, vb, taps)
    cells = c * (-(-h // vq.TILE) * vq.TILE) * (-(-w // vq.TILE) * vq.TILE) if padded_count else c * h * w
    per_stack = lambda g: (np.asarray(g, np.float32).T.reshape(NVIEW * n) / np.float32(cells)).reshape(-1, 1, 1, 1)    # stack index = viewport * n + image
    gm, gs = per_stack(g_mse), per_stack(g_ssim)
    b_pa, b_pb, b_q, b_r = (_blur_t(np.ascontiguousarray(x, np.float32), taps, r, reverse, halo, padding) for x in coefs)
    two, qf = np.float32(2), np.float32(q_factor)
    t = b_pa + (qf * va) * b_q
    t = t + vb * b_r
    gva = gs * t + gm * (two * (va - vb))
    t = b_pb + (qf * vb) * b_q
    t = t + va * b_r
    gvb = gs * t + gm * (two * (vb - va))
    assert gva.dtype == np.float32 and gvb.dtype == np.float32
    return gva, gvb


def torch_quality(ta, tb, taps):
    """f64_quality's formula (the 2-D window, zero padding) on torch tensors [14 n, c, h, w] of any float dtype: (mse, ssim), each [14 n]"""
    import torch
    import torch.nn.functional as F
    t = torch.as_tensor(np.asarray(taps, np.float64)).to(ta.dtype)
    ch, k = ta.shape[1], len(taps)
    win = (t[:, None] * t[None, :]).expand(ch, 1, k, k).contiguous()
    blur = lambda x: F.conv2d(x, win, padding=k // 2, groups=ch)
    mu_a, mu_b = blur(ta), blur(tb)
    var_a, var_b, cov = blur(ta * ta) - mu_a * mu_a, blur(tb * tb) - mu_b * mu_b, blur(ta * tb) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    return ((ta - tb) ** 2).mean(dim=(1, 2, 3)), m.mean(dim=(1, 2, 3))


def torch_loss(mse, ssim, g_mse, g_ssim):
    """sum of upstream * value over (image, viewport), the scalar whose gradient the backward computes; mse, ssim [14 n] in stack order"""
    import torch
    n = mse.shape[0] // NVIEW
    g = lambda x: torch.as_tensor(np.asarray(x, np.float64).T.reshape(NVIEW * n).copy()).to(mse.dtype)
    return (g(g_mse) * mse).sum() + (g(g_ssim) * ssim).sum()


def torch_view_grads(va, vb, taps, g_mse, g_ssim, dtype="float64"):
    """(gva, gvb) by torch autograd on the CPU: float64 is the reference, float32 (the library's convolution and its backward) the yardstick"""
    import torch
    ta, tb = (torch.tensor(np.ascontiguousarray(v), dtype=getattr(torch, dtype), requires_grad=True) for v in (va, vb))
    torch_loss(*torch_quality(ta, tb, taps), g_mse, g_ssim).backward()
    return ta.grad.numpy(), tb.grad.numpy()


def sample_terms(tf, hs, ws, near):
    """the ERP cells and fp32 weights lic360_project_sample reads / lic360_project_scatter adds to, from a table tf [14, h_out * w_out, 2] fp32:
    a list of (index into one plane [14, inner] int64, weight [14, inner] fp32 or None for weight 1)"""
    tf = np.asarray(tf, np.float32)
    fx, fy = tf[..., 0], tf[..., 1]
    if near:
        tw = np.floor(fx.astype(np.float64) + 0.5).astype(np.int64) % ws
        th = np.minimum(np.floor(fy.astype(np.float64) + 0.5).astype(np.int64), hs - 1)
        return [(th * ws + tw, None)]
    tw, th = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    pw, ph = (tw + 1) % ws, np.minimum(th + 1, hs - 1)
    tx, ty = fx - tw.astype(np.float32), fy - th.astype(np.float32)
    ntx, nty = (1.0 - tx.astype(np.float64)).astype(np.float32), (1.0 - ty.astype(np.float64)).astype(np.float32)
    return [(th * ws + tw, ntx * nty), (th * ws + pw, tx * nty), (ph * ws + tw, ntx * ty), (ph * ws + pw, tx * ty)]


def scatter_sums(tf, gv, n, c, hs, ws, near):
    """(sum, sum of magnitudes, number of terms), each [n, c, hs, ws] (float64, float64, int64), of the fp32 products the backward kernel adds into
    each ERP cell for the view gradients gv [14 n, c, h_out, w_out] fp32"""
    g = np.ascontiguousarray(gv, np.float32).reshape(NVIEW, n * c, -1)
    plane, size = (np.arange(n * c, dtype=np.int64) * hs * ws)[None, :, None], n * c * hs * ws
    total, mag, count = np.zeros(size), np.zeros(size), np.zeros(size, np.int64)
    for idx, wgt in sample_terms(tf, hs, ws, near):
        prod = g if wgt is None else wgt[:, None, :] * g
        assert prod.dtype == np.float32
        flat = (plane + idx[:, None, :]).ravel()
        total += np.bincount(flat, weights=prod.ravel().astype(np.float64), minlength=size)
        mag += np.bincount(flat, weights=np.abs(prod).ravel().astype(np.float64), minlength=size)
        count += np.bincount(flat, minlength=size)
    return tuple(x.reshape(n, c, hs, ws) for x in (total, mag, count))
