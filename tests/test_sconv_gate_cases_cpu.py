"""tests/sconv_gate_cases.py checked by itself, without a GPU: the case list reaches the six gate kernels; the exactness condition holds for every case, form
and tier; the pre-activations sit inside the sigmoid's working range (conditions on the data, not tolerances); the saturation case holds each special channel
kind; every mutation -- a bug the epilogue could have -- changes the reference; the reference leaves the frame at the sentinel; and on the real-valued data
of the GPU parity test the stated bound passes the kernel's arithmetic done on the host and fails the same arithmetic with g rounded to bf16."""
import numpy as np
import pytest

import sconv_cases as sc
import sconv_gate_cases as gc


def test_the_case_list_reaches_the_six_kernels():
    assert {gc.instantiation(c, f) for c in gc.CASES for f in gc.FORMS} == {(f, nq) for f in gc.FORMS for nq in (4, 2)}
    assert all(c.ks == 1 and c.crop == 0 and not c.shuffle and not c.slope and sc.supported(True, c.cin, c.cout, 1) for c in gc.CASES)
    br = {c.name: gc.branch_of(c, True) for c in gc.CASES}
    assert br["g_q4_one"].chunks == 1 and (br["g_q4_one"].tiles_y, br["g_q4_one"].tiles_x) == (1, 2)
    assert br["g_q4_ragged_n3"].chunks == 2 and gc.BY_NAME["g_q4_ragged_n3"].n == 3
    assert br["g_q4_low"].full == 0 and br["g_q2_low"].full == 0
    assert br["g_q4_3rows"].tiles_y == 3 and br["g_q4_3rows"].chunks == 6 and br["g_q2_3rows"].tiles_y == 3
    assert br["g_q4_blocks"].blocks_y == 2 and br["g_q2"].nq == 2
    assert (gc.BY_NAME["g_prod_132x260"].hp, gc.BY_NAME["g_prod_132x260"].wp, gc.BY_NAME["g_prod_132x260"].n) == (132, 260, 1)
    assert len(gc.PARAMS) == 7 * len(gc.CASES)


@pytest.mark.parametrize("p", gc.PARAMS, ids=gc.ident)
def test_exactness_and_the_conditions_on_y(p):
    case, form, tier = p
    data, want = gc.shared(case, form, tier)
    assert gc.assert_exact_domain(case, form, tier, data) < sc.EXACT_BELOW
    y = gc.conv_y(case, form, data)                                         # (asserts that y is an fp32 number)
    assert np.array_equal(y * np.float32(2.0 ** data["s"]), np.rint(y * np.float32(2.0 ** data["s"])))
    normal = np.ones(case.cout, bool)
    if case.name == "g_saturate":
        for bias, chans in gc.SATURATE.items():
            normal[list(chans)] = False
            assert (y[:, list(chans)] == np.float32(bias)).all()
            g = gc.sigmoid32(y[:, list(chans)])
            assert (g == {64.0: 1.0, -128.0: 0.0}[bias]).all() if bias else (np.unique(g).size == 1 and 0.4 < float(g.flat[0]) < 0.6)
        assert all(len(v) >= 2 for v in gc.SATURATE.values())
    yn = y[:, normal]
    share, top = float((np.abs(yn) < 8).mean()), float(np.abs(yn).max())
    print("%s: s = %d, share of |y| < 8: %.3f, max |y| %.2f" % (gc.ident(p), data["s"], share, top))
    assert share >= 0.9 and top <= 32 and (yn > 0).any() and (yn < 0).any()
    # the frame of the reference is the sentinel, the window is not all sentinel
    frame = np.ones(want.shape, bool)
    frame[gc.window(case)] = False
    assert (want[frame] == gc.SENTINEL).all() and frame.any() and want.dtype == np.float32 and np.isfinite(want).all()


FP_SMALL = [(c, f, gc.TIERS[f][0]) for c in gc.SMALL for f in gc.FORMS]


@pytest.mark.parametrize("p", FP_SMALL, ids=gc.ident)
def test_every_mutation_changes_the_reference(p):
    case, form, tier = p
    data, want = gc.shared(case, form, tier)
    muts = [m for m, applies in gc.MUTATIONS.items() if applies(case)]
    assert len(muts) >= 7
    for m in muts:
        got = gc.reference(case, form, data, m)
        assert got.shape == want.shape and not np.array_equal(got, want), "%s: mutation %s is invisible" % (gc.ident(p), m)
        if m not in ("row_shift", "col_shift"):                             # an arithmetic bug shows on the window itself
            assert not np.array_equal(got[gc.window(case)], want[gc.window(case)]), (gc.ident(p), m)


def test_every_mutation_applies_somewhere():
    assert set(gc.MUTATIONS) == {"trunk_res_swapped", "exp_plus", "bias_after_sigmoid", "fma", "block_trunk", "row_shift", "col_shift", "g_bf16"}
    for m, applies in gc.MUTATIONS.items():
        assert any(applies(c) for c in gc.SMALL), m


@pytest.mark.parametrize("name", gc.REAL_CASES)
def test_the_parity_bound_passes_the_arithmetic_and_fails_a_bf16_gate(name):
    case = gc.BY_NAME[name]
    d = gc.real_data(case)
    ops = (d["x"], d["w"], d["b"], d["trunk"], d["res"])
    for form in ("fp32", "bf16x1"):
        want = gc.gate64(*ops, form=form)
        good, bad = gc.parity_excess(gc.emulate32(*ops, form=form), want, d["trunk"], d["res"]), gc.parity_excess(gc.emulate32(*ops, form=form, mut="g_bf16"), want, d["trunk"], d["res"])
        print("%s / %s: excess over the bound %.3g (reference arithmetic), %.3g (g rounded to bf16)" % (name, form, good, bad))
        assert good <= 0 < bad
    assert gc.parity_excess(gc.emulate32(*ops, form="bf16x1"), gc.gate64(*ops), d["trunk"], d["res"]) > 0      # the forms are distinct on this data
