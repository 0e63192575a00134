"""tests/viewport_quality_cases.py checked by itself (no GPU): the fp32 restatement of the fused viewport metrics lies as close to a float64
evaluation as the library's fp32 SSIM does, gives exactly 1 / 0 on identical inputs, and notices three plausible kernel mistakes."""
import numpy as np
import pytest

import viewport_quality_cases as vq


@pytest.fixture(scope="module")
def evaluated():
    """per case: the view stacks, the restatement, float64 and the library's fp32 evaluation -- computed once"""
    out = {}
    for case in vq.CASES:
        va, vb = vq.make_view_pair(case)
        taps = vq.taps_of(case.window)
        out[case.name] = (va, vb, taps, vq.ref_quality(va, vb, taps), vq.f64_quality(va, vb, taps), vq.library_quality(va, vb, case.window))
    return out


def test_cases_cover_what_the_kernel_branches_on():
    views = {c.view for c in vq.CASES}
    assert {(16, 16), (21, 37), (5, 7), (171, 256)} <= views
    assert {c.n for c in vq.CASES} >= {1, 3} and {c.c for c in vq.CASES} >= {1, 3}
    assert any(c.near and c.view == (21, 37) for c in vq.CASES) and any(c.window == 3 for c in vq.CASES) and any(c.kind == "noise" for c in vq.CASES)
    for c in vq.CASES:
        t = vq.taps_of(c.window)
        assert t.dtype == np.float32 and len(t) == c.window and abs(float(t.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(t, t[::-1])


def test_restatement_is_as_close_to_float64_as_the_library_ssim(evaluated):
    """the yardstick is the deviation of lic360_operator.SSIM (fp32, CPU, library convolution) and of torch's fp32 mean from float64 on the same
    inputs; the restatement may deviate at most 4 times as much (the separable and the 2-D order round differently, neither is privileged)"""
    dev = {"ssim": [0.0, 0.0], "mse": [0.0, 0.0]}
    for name, (va, vb, taps, (mse, ssim, _), (mse64, ssim64), (mse_lib, ssim_lib)) in evaluated.items():
        for key, mine, lib, ref in (("ssim", ssim, ssim_lib, ssim64), ("mse", mse, mse_lib, mse64)):
            d = [float(np.abs(x.astype(np.float64) - ref).max()) for x in (mine, lib)]
            print("%-20s %-4s restatement %.3e  library %.3e" % (name, key, d[0], d[1]))
            dev[key] = [max(dev[key][0], d[0]), max(dev[key][1], d[1])]
            assert d[1] > 0 and d[0] <= 4 * d[1], (name, key, d)                     # case by case (the values of the cases differ in size) ...
    print("all cases: ssim restatement %.3e library %.3e   mse restatement %.3e library %.3e" % (dev["ssim"][0], dev["ssim"][1], dev["mse"][0], dev["mse"][1]))
    for key, (mine, lib) in dev.items():
        assert lib > 0 and mine <= 4 * lib, (key, mine, lib)                          # ... and over all of them


@pytest.mark.parametrize("case", vq.CASES, ids=[c.name for c in vq.CASES])
def test_identical_inputs_give_exactly_one_and_zero(case):
    """2 mu mu and mu mu + mu mu are the same fp32 number, so numerator and denominator are equal bit for bit; sums of ones below 2^24 are exact"""
    va, _ = vq.make_view_pair(case)
    mse, ssim, m = vq.ref_quality(va, va.copy(), vq.taps_of(case.window))
    assert mse.shape == ssim.shape == (case.n, vq.NVIEW) and m.shape == va.shape
    assert np.all(m == 1.0) and np.all(ssim == 1.0) and np.all(mse == 0.0)


@pytest.mark.parametrize("mutation", [dict(padding="reflect"), dict(halo=4), dict(padded_count=True)], ids=["reflect_padding", "halo_4", "padded_count"])
def test_restatement_notices_kernel_mistakes(evaluated, mutation):
    changed = []
    for case in vq.CASES:
        if case.view == (171, 256):
            continue                                                                  # (the small cases already decide; keeps the test quick)
        va, vb, taps, (mse, ssim, m) = evaluated[case.name][:4]
        mse2, ssim2, m2 = vq.ref_quality(va, vb, taps, **mutation)
        if not (np.array_equal(ssim, ssim2) and np.array_equal(mse, mse2)):
            changed.append(case.name)
    assert changed, mutation
    if "halo" in mutation:                                                            # the window of 3 lies inside a halo of 4: that case must not change
        assert "partial_tiles_win3" not in changed and "partial_tiles" in changed
    if "padded_count" in mutation:                                                    # 16 x 16 is its own padded tile
        assert "one_tile" not in changed and "partial_tiles" in changed
