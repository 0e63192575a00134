"""The cases of the fused GMM rate loss (tests/gmm_rate_cases.py) without a GPU: the case list reaches every path of the restated launch
geometry, the restated constants are the source's, the reference agrees with the float64 statement of the head within the recorded figures,
and every model of a broken kernel changes the reference on some case.

The library composition of lic360_operator.GmmRateLoss is NOT testable here: `lic360` (and with it lic360_operator) computes nothing without the
device library's kernels; tests/test_gpu_gmm_rate.py holds it against the same float64 statement on the GPU."""
import os
import re

import numpy as np
import pytest

import gmm_rate_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "360-image-compression_amd", "csrc", "gmm_rate_kernels.hip")


def test_restated_constants_are_the_source_s():
    text = open(SOURCE).read()
    m = re.search(r"constexpr int GR_THREADS = (\d+), GR_PER_THREAD = (\d+), GR_CHUNK = GR_THREADS \* GR_PER_THREAD, GR_MAX_NG = (\d+);", text)
    assert m, "the kernel's constants are no longer stated as the cases file restates them"
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (gc.THREADS, gc.PER_THREAD, gc.MAX_NG) and gc.CHUNK == gc.THREADS * gc.PER_THREAD
    assert re.search(r"constexpr float GR_SIGMA_FLOOR = 0\.00001f;", text) and gc.SIGMA_FLOOR == np.float32(0.00001)
    assert "if (ng == %d && vec)" % gc.STATIC_NG in text                    # the one mixture size with an instantiation of its own
    assert "w % 4 == 0 && aligned16(logit)" in text                        # the vector form's condition starts as restated in form()
    assert "bool aligned16(const void *p) { return plane_walk_aligned(p, 4 * GR_PER_THREAD); }" in text and 4 * gc.PER_THREAD == 16


def test_case_ids_are_unique_and_cases_reach_every_path():
    assert len(gc.BY_ID) == len(gc.CASES)
    reached = set()
    for case in gc.CASES:
        reached |= gc.reach(case)
    assert set(gc.REACH) <= reached, sorted(set(gc.REACH) - reached)
    for family in (gc.REGULAR, gc.EDGE):                                     # both instantiations and both forms in either family
        assert {(gc.form(c), gc.instantiation(c)) for c in family} == {(f, i) for f in ("vec", "scalar") for i in ("static", "generic")}
    assert {c.ng for c in gc.CASES} == {1, 3, 5}
    named = {(c.N, c.G, c.H, c.W) for c in gc.CASES}
    assert {(1, 1, 1, 1), (3, 5, 3, 5), (2, 4, 6, 8), (2, 3, 4, 12)} <= named
    assert any(c.offset % 4 and c.W % 4 == 0 and gc.form(c) == "scalar" for c in gc.CASES)


def test_edge_cases_hold_the_values_they_are_for():
    for case in gc.EDGE:
        d, ref = gc.inputs(case), gc.reference(case)
        coded = ref["coded"]
        cc = np.repeat(coded, case.ng, 1)
        s = d["sigma"][cc]
        assert (s == 0).any() and (s < 0).any() and np.signbit(s[s == 0]).any() and ((s < 0) & (s + gc.SIGMA_FLOOR > 0)).any(), case.id
        L = gc.rows(d["logit"], case)[coded.reshape(-1)]
        assert (L == L[:, :1]).all(1).any(), case.id                                         # equal logits
        if case.ng > 1:
            assert (gc.softmax_rows(L) == 0).any(), case.id                                  # a weight that is exactly 0
        assert (ref["map"][coded] == gc.GMM_UNDERFLOW_LOSS).any(), case.id                   # p underflowed: -log(1e-7)
        lab = d["label"][coded]
        assert (lab == -3.5).any() and (lab == 3.5).any(), case.id
        m = d["mask"]
        assert (m == 0.5).any() and (m == np.nextafter(np.float32(0.5), np.float32(0))).any() and (m > 1).any(), case.id
        for k in ("logit", "sigma", "mean"):
            assert np.isfinite(d[k][cc]).all() and not np.isfinite(d[k][~cc]).all(), (case.id, k)    # Inf / NaN under uncoded symbols only
        assert np.isfinite(d["label"][coded]).all()
        for k in ("map", "d_logit", "d_sigma", "d_mean", "d_label"):
            assert np.isfinite(ref[k]).all(), (case.id, k)
            assert not ref[k][~(cc if ref[k].shape[1] != case.G else coded)].any(), (case.id, k)     # exact zeros where uncoded
    grads = np.concatenate([gc.inputs(c)["grad"] for c in gc.EDGE])
    assert (grads == 0).any() and (grads < 0).any() and (grads > 0).any()
    assert any(len(set(gc.inputs(c)["grad"].tolist())) > 1 for c in gc.EDGE)


def test_masked_out_cases_cost_nothing():
    for case in gc.CASES:
        ref, d = gc.reference(case), gc.inputs(case)
        if case.mask == "zeros":
            assert not ref["nats"].any() and not ref["symbols"].any() and not any(ref[k].any() for k in ("map", "d_logit", "d_sigma", "d_mean", "d_label"))
        if case.mask == "image":
            assert ref["symbols"][1] == 0 and ref["nats"][1] == 0 and not ref["d_logit"][1].any() and ref["symbols"][0] == case.G * case.H * case.W
        if case.mask in ("absent", "ones"):
            assert (ref["symbols"] == case.G * case.H * case.W).all()
        assert (ref["symbols"] == gc.coded_of(d["mask"], case).reshape(case.N, -1).sum(1)).all()


def test_fmaf_is_the_fused_operation():
    """against exact rational arithmetic rounded once (independent_tables.fmaf), on operands chosen to sit near rounding ties"""
    import independent_tables as it
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, 4000).astype(np.float32)
    b = rng.normal(0, 1, 4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    c[::3] = rng.normal(0, 1, len(c[::3])).astype(np.float32)
    got = gc.fmaf(a, b, c)
    want = np.array([it.fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", gc.REGULAR, ids=lambda c: c.id)
def test_reference_against_float64(case):
    """the restatement against the float64 statement on the rows with p >= GMM_MIN_P; prints the measurement, holds the recorded tolerance and
    holds it within a factor 2 of the measurement; the draw keeps at least GMM_MIN_KEPT of the coded symbols"""
    ref = gc.reference(case)
    worst, dn, share, scale = gc.f64_distance(case, ref)
    print("%s: gradients / loss %.3g at gradient scale %.3g, nats %.3g, %.1f %% of the coded rows kept" % (case.id, worst, scale, dn, 100 * share))
    assert share >= gc.GMM_MIN_KEPT, "change the draw, not the cap"
    tol, tol_n = gc.F64_TOL[case.id]
    assert worst <= tol and dn <= tol_n
    assert tol <= 2 * worst or worst == 0 == tol
    assert tol_n <= 2 * dn or (dn == 0 and tol_n <= 2.0 ** -40)


@pytest.mark.parametrize("broken", gc.BROKEN)
def test_every_broken_model_changes_the_reference(broken):
    changed = []
    for case in gc.CASES:
        ref, bad = gc.reference(case), gc.reference(case, broken)
        if any(ref[k].tobytes() != bad[k].tobytes() for k in ("map", "symbols", "nats", "d_logit", "d_sigma", "d_mean", "d_label")):
            changed.append(case.id)
    print(broken, "changes", len(changed), "cases")
    assert changed, "no case would notice a kernel that is broken this way"
    if broken == "finish_first_pass_only":                                   # only an image of more than THREADS slots can show it
        assert changed == [c.id for c in gc.SLOTS] and len(changed) == 2
