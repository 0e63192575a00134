"""Cases and an fp32 restatement of the fused viewport metrics (csrc/viewport_quality_kernels.hip, lic360.viewport_quality).  No GPU in here:
tests/test_viewport_quality_cases_cpu.py checks this file by itself, tests/test_gpu_viewport_quality.py compares the kernel with it.

ref_quality(va, vb, taps) restates what the kernel does to the two stacks of projected views [14 n, c, h, w] (viewport-major, the output of
ProjectsOp.forward), in numpy fp32, one rounding per operation:
  * zero padding of len(taps) // 2 cells a side;
  * the window as a row pass then a column pass over a, b, a*a, b*b, a*b, taps in ascending order from a zero accumulator, each tap one
    rounded product and one rounded sum;
  * SSIM per cell in the operation order of lic360_operator/extras.py (SSIM.map), c1 and c2 rounded to fp32 as torch's tensor-scalar sum does;
  * float64 sums of the fp32 cells per (image, viewport), divided by c*h*w and rounded to fp32.
Its keyword arguments switch in the three kernel mistakes tests/test_viewport_quality_cases_cpu.py shows it is sensitive to.

Deviation from float64, measured by tests/test_viewport_quality_cases_cpu.py over all the cases below (float64 evaluation of the same formula
with the 2-D window, on the same view stacks; largest absolute difference of a per-viewport value):
    SSIM: restatement 8.1e-08, lic360_operator.SSIM (CPU, library convolution) 1.25e-07       MSE: restatement 7.9e-09, torch fp32 mean 2.8e-08
(the yardstick is the second number of each pair; the restatement is allowed 4x that)."""
import collections

import numpy as np

NVIEW, TILE = 14, 16
Case = collections.namedtuple("Case", "name erp view n c near window kind seed fov", defaults=(0.5,))
# ERP h x w, viewport h x w: the smallest at which the kernel can go wrong
CASES = [
    # (fov 0.4: at the 0.5 of the other cases a square viewport's half height is 45 degrees, so the top row of the views pitched by 45 degrees looks exactly
    # at a pole, where the table's longitude is undefined and leaves the ERP -- tests/test_gpu_viewport_quality.py checks every table before it samples)
    Case("one_tile", (32, 64), (16, 16), 1, 3, False, 11, "uniform", 1, 0.4),           # one exact tile
    Case("partial_tiles", (32, 64), (21, 37), 3, 3, False, 11, "uniform", 2),           # partial tiles both ways, every border tile sees padding
    Case("partial_tiles_near", (32, 64), (21, 37), 1, 1, True, 11, "uniform", 3),       # nearest-neighbour sampling
    Case("partial_tiles_win3", (32, 64), (21, 37), 1, 3, False, 3, "uniform", 4),       # a window smaller than the kernel's largest
    Case("below_radius", (32, 64), (5, 7), 3, 1, False, 11, "uniform", 5),              # a viewport smaller than the window radius on one side
    Case("production", (64, 128), (171, 256), 1, 3, False, 11, "noise", 6),             # 171 = 10 * 16 + 11 rows, 16 exact tile columns; b = a + noise
]


def taps_of(window):
    """the fp32 1-D window of lic360_operator.extras (whose outer product is SSIM's 2-D window)"""
    from lic360_operator.extras import _gauss_taps
    return _gauss_taps(window).numpy().astype(np.float32)


def _pair(shape, kind, seed):
    rng = np.random.default_rng(seed)
    a = rng.random(shape, dtype=np.float32)
    b = rng.random(shape, dtype=np.float32) if kind == "uniform" else (a + np.float32(0.02) * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return a, b


def make_erp_pair(case):
    """the ERP batches a, b [n, c, H, W] fp32 of a case: uniform in [0, 1), or b = a + noise of sigma 0.02 (the regime of a decoded image)"""
    return _pair((case.n, case.c) + case.erp, case.kind, case.seed)


def make_view_pair(case):
    """view stacks [14 n, c, h, w] of the same statistics, for the tests that have no device to project with"""
    return _pair((NVIEW * case.n, case.c) + case.view, case.kind, case.seed)


def _window_pass(p, taps, h, w):
    """p [..., h + 2r, w + 2r] zero-padded -> [..., h, w]: rows then columns, ascending taps from zero, separate fp32 multiply and add"""
    acc = np.zeros(p.shape[:-1] + (w,), np.float32)
    for k, t in enumerate(taps):
        acc = acc + np.float32(t) * p[..., k:k + w]
    out = np.zeros(p.shape[:-2] + (h, w), np.float32)
    for k, t in enumerate(taps):
        out = out + np.float32(t) * acc[..., k:k + h, :]
    return out


def _ssim_cells(pa, pb, taps, h, w):
    two, c1, c2 = np.float32(2), np.float32(0.01 ** 2), np.float32(0.03 ** 2)
    mu_a, mu_b = _window_pass(pa, taps, h, w), _window_pass(pb, taps, h, w)
    e_aa, e_bb, e_ab = _window_pass(pa * pa, taps, h, w), _window_pass(pb * pb, taps, h, w), _window_pass(pa * pb, taps, h, w)
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    m = ((two * mu_a * mu_b + c1) * (two * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    assert m.dtype == np.float32
    return m


def ref_quality(va, vb, taps, padding="zero", halo=None, padded_count=False):
    """(mse [n, 14], ssim [n, 14], map [14 n, c, h, w]) of two view stacks [14 n, c, h, w] fp32.  The keyword arguments are kernel mistakes:
    padding="reflect" mirrors the views at their border; halo=k gathers only k cells around each 16 x 16 tile (taps beyond read 0);
    padded_count divides by the cells of the whole tiles."""
    va, vb, taps = np.ascontiguousarray(va, np.float32), np.ascontiguousarray(vb, np.float32), np.asarray(taps, np.float32)
    assert va.shape == vb.shape and va.ndim == 4 and va.shape[0] % NVIEW == 0 and len(taps) % 2 == 1
    n, (c, h, w), r = va.shape[0] // NVIEW, va.shape[1:], len(taps) // 2
    pad = ((0, 0), (0, 0), (r, r), (r, r))
    pa, pb = (np.pad(v, pad, mode="reflect") if padding == "reflect" and r else np.pad(v, pad) for v in (va, vb))
    if halo is None:
        m = _ssim_cells(pa, pb, taps, h, w)
    else:                                        # tile by tile, as the kernel works: what lies more than `halo` cells outside the tile reads 0
        m, cut = np.zeros(va.shape, np.float32), max(r - halo, 0)
        for y0 in range(0, h, TILE):
            for x0 in range(0, w, TILE):
                th, tw = min(TILE, h - y0), min(TILE, w - x0)
                qa, qb = (p[..., y0:y0 + th + 2 * r, x0:x0 + tw + 2 * r].copy() for p in (pa, pb))
                for q in (qa, qb):
                    if cut:
                        q[..., :cut, :] = 0
                        q[..., -cut:, :] = 0
                        q[..., :, :cut] = 0
                        q[..., :, -cut:] = 0
                m[..., y0:y0 + th, x0:x0 + tw] = _ssim_cells(qa, qb, taps, th, tw)
    d = va - vb
    cells = c * (-(-h // TILE) * TILE) * (-(-w // TILE) * TILE) if padded_count else c * h * w
    per_view = lambda t: (t.astype(np.float64).sum(axis=(1, 2, 3)) / cells).astype(np.float32).reshape(NVIEW, n).T.copy()
    return per_view(d * d), per_view(m), m


def f64_quality(va, vb, taps):
    """the same formula in float64 with the 2-D window (the outer product of the taps): (mse [n, 14], ssim [n, 14]) as float64"""
    from scipy import ndimage
    va, vb, t = np.asarray(va, np.float64), np.asarray(vb, np.float64), np.asarray(taps, np.float64)
    n, win = va.shape[0] // NVIEW, (t[:, None] * t[None, :])[None, None]
    blur = lambda x: ndimage.correlate(x, win, mode="constant", cval=0.0)
    mu_a, mu_b = blur(va), blur(vb)
    var_a, var_b, cov = blur(va * va) - mu_a * mu_a, blur(vb * vb) - mu_b * mu_b, blur(va * vb) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    per_view = lambda x: x.mean(axis=(1, 2, 3)).reshape(NVIEW, n).T.copy()
    return per_view((va - vb) ** 2), per_view(m)


def library_quality(va, vb, window):
    """lic360_operator.SSIM (fp32, the library's convolution) and torch's fp32 mean on the CPU: (mse [n, 14], ssim [n, 14]); the yardstick of
    how far an fp32 evaluation of this formula lies from float64"""
    import torch
    from lic360_operator.extras import SSIM
    ta, tb, n = torch.from_numpy(np.ascontiguousarray(va)), torch.from_numpy(np.ascontiguousarray(vb)), va.shape[0] // NVIEW
    ssim = SSIM(window, ta.shape[1], size_average=False)(ta, tb)
    mse = ((ta - tb) ** 2).mean(dim=(1, 2, 3))
    return mse.view(NVIEW, n).t().numpy().copy(), ssim.view(NVIEW, n).t().numpy().copy()
