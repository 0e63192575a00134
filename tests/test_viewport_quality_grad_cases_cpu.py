"""tests/viewport_quality_grad_cases.py checked by itself (no GPU): the fp32 restatement of the fused viewport metrics' backward lies as close to
a float64 autograd of the same formula as torch's own fp32 autograd does, its scatter helper adds up to the adjoint of the sampling, and it notices
five plausible kernel mistakes, each on the case meant for it."""
import numpy as np
import pytest

import viewport_quality_cases as vq
import viewport_quality_grad_cases as vg


@pytest.fixture(scope="module")
def evaluated():
    """per case: view stacks, taps, upstream gradients, the maps and view gradients of the restatement -- computed once"""
    out = {}
    for case in vg.CASES:
        va, vb = vq.make_view_pair(case)
        taps, (g_mse, g_ssim) = vg.taps_of(case), vg.upstream(case)
        coefs = vg.ref_coefs(va, vb, taps)
        out[case.name] = dict(va=va, vb=vb, taps=taps, g_mse=g_mse, g_ssim=g_ssim, coefs=coefs, grads=vg.ref_view_grads(va, vb, taps, coefs, g_mse, g_ssim))
    return out


def test_cases_are_the_forwards_and_one_with_asymmetric_taps():
    assert vg.CASES[:len(vq.CASES)] == list(vq.CASES) and len(vg.CASES) == len(vq.CASES) + 1
    asym = vg.CASES[-1]
    t = vg.taps_of(asym)
    assert asym.view in {c.view for c in vq.CASES} and asym.erp in {c.erp for c in vq.CASES}
    assert t.dtype == np.float32 and len(t) == asym.window and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6 and not np.array_equal(t, t[::-1])
    for case in vg.CASES:
        g_mse, g_ssim = vg.upstream(case)
        assert g_mse.shape == g_ssim.shape == (case.n, vg.NVIEW) and (g_mse == 0).sum() == 1 and (g_ssim == 0).sum() == 1
        assert (g_mse < 0).any() and (g_mse > 0).any() and (g_ssim < 0).any() and (g_ssim > 0).any()


def test_restatement_is_as_close_to_float64_as_torchs_fp32_autograd(evaluated):
    """the yardstick is torch's fp32 autograd of the same formula on the CPU (the library's convolution, forward and backward) against float64 on
    the same views, over the largest float64 gradient of the case; the restatement may deviate 4 times as much (it orders the sums differently)"""
    worst = [0.0, 0.0]
    for case in vg.CASES:
        e = evaluated[case.name]
        args = (e["va"], e["vb"], e["taps"], e["g_mse"], e["g_ssim"])
        ref, lib = vg.torch_view_grads(*args), vg.torch_view_grads(*args, dtype="float32")
        scale = max(float(np.abs(x).max()) for x in ref)
        mine, yard = (max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(g, ref)) / scale for g in (e["grads"], lib))
        print("%-20s restatement %.3e  torch fp32 %.3e  (largest float64 gradient %.3e)" % (case.name, mine, yard, scale))
        worst = [max(worst[0], mine), max(worst[1], yard)]
        assert scale > 0 and yard > 0 and mine <= 4 * yard, (case.name, mine, yard)
    print("all cases: restatement %.3e  torch fp32 %.3e" % tuple(worst))


def test_an_upstream_zero_leaves_only_the_other_metric(evaluated):
    """where g_ssim is exactly 0 the view gradient is the MSE term alone, bit for bit (gs * t is a signed zero)"""
    case = vg.CASES[1]
    e = evaluated[case.name]
    s = 3 * case.n + 0                                                               # upstream() zeroes g_ssim[0, 3]: stack index viewport * n + image
    gm = np.float32(e["g_mse"][0, 3]) / np.float32(case.c * case.view[0] * case.view[1])
    assert np.array_equal(e["grads"][0][s], gm * (np.float32(2) * (e["va"][s] - e["vb"][s])))


def test_scatter_helper_is_the_adjoint_of_the_sampling():
    """<project(x), g> == <x, scatter(g)> in float64 up to the fp32 rounding of the products, on a table that wraps around the ERP's seam and clamps
    at its last row; term counts: four per view cell, one with nearest sampling"""
    rng = np.random.default_rng(11)
    n, c, hs, ws, inner = 2, 2, 8, 16, 40
    tf = np.stack([rng.random((vg.NVIEW, inner), dtype=np.float32) * np.float32(ws - 0.01), rng.random((vg.NVIEW, inner), dtype=np.float32) * np.float32(hs - 0.51)], axis=-1)
    x, g = rng.standard_normal((n * c, hs * ws)), rng.standard_normal((vg.NVIEW * n, c, 5, 8)).astype(np.float32)
    for near in (False, True):
        terms = vg.sample_terms(tf, hs, ws, near)
        assert all(idx.min() >= 0 and idx.max() < hs * ws for idx, _ in terms)
        assert any((idx % ws == 0).any() for idx, _ in terms) and any((idx // ws == hs - 1).any() for idx, _ in terms)
        views = sum(x[:, idx].transpose(1, 0, 2) * (1.0 if wgt is None else wgt.astype(np.float64)[:, None, :]) for idx, wgt in terms)     # [14, n c, inner]
        total, mag, count = vg.scatter_sums(tf, g, n, c, hs, ws, near)
        lhs, rhs = float((views * g.reshape(vg.NVIEW, n * c, inner)).sum()), float((x.reshape(n, c, hs, ws) * total).sum())
        assert abs(lhs - rhs) <= 1e-6 * float((np.abs(x).reshape(n, c, hs, ws) * mag).sum())
        assert int(count.sum()) == len(terms) * g.size and (mag[count == 0] == 0).all() and (np.abs(total) <= mag * (1 + 1e-12)).all()


MISTAKES = {
    "unreversed_taps": dict(reverse=False),
    "halo_4": dict(halo=4),
    "mirrored_outside": dict(padding="reflect"),
    "padded_count": dict(padded_count=True),
    "no_factor_2_on_q": dict(q_factor=1),
}


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_restatement_notices_kernel_mistakes(evaluated, mistake):
    changed = []
    for case in vg.CASES:
        if case.view == (171, 256):
            continue                                                                  # (the small cases already decide; keeps the test quick)
        e = evaluated[case.name]
        wrong = vg.ref_view_grads(e["va"], e["vb"], e["taps"], e["coefs"], e["g_mse"], e["g_ssim"], **MISTAKES[mistake])
        if not all(np.array_equal(x, y) for x, y in zip(wrong, e["grads"])):
            changed.append(case.name)
    if mistake == "unreversed_taps":                                                  # a symmetric window is its own reverse: only the asymmetric case can tell
        assert changed == ["asymmetric_taps"]
    elif mistake == "halo_4":                                                         # the window of 3 lies inside a halo of 4
        assert "partial_tiles" in changed and "asymmetric_taps" in changed and "partial_tiles_win3" not in changed
    elif mistake == "padded_count":                                                   # 16 x 16 is its own padded tile
        assert "partial_tiles" in changed and "one_tile" not in changed
    else:
        assert len(changed) == len(vg.CASES) - 1, changed
